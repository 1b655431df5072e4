// fl_jpeg_opt_core.h -- per-picture Huffman tables of the JPEG encoder (FLGPU_FEO_JPEG_OPTIMIZE on FLGPU_FE_JPEG): the rule that turns a
// table's symbol counts into code lengths, canonical codes and a DHT segment, and the never-larger decision, as code that compiles for
// the host and for the device.  fl_jpeg_opt.hip (jpeg_opt_tables_kernel) runs it over a workgroup, flgpu_debug_jpeg_optimize_tables
// (fl_encode.cpp) in plain loops, tests/jpeg_opt_model.py restates it.
//
// The rule, integer only, per table (DHT order: 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma).  Input: count[256], the number of
// times the picture's scan codes each symbol; the sum of a table's counts is below 2^32 - 1.
//   1. the leaves are the used symbols (count > 0) and one reserved leaf of count 1, in ascending (count, symbol) order, the
//      reserved leaf in front of every symbol (jpeg_opt_before, jpeg_opt_rank);
//   2. minimum-redundancy depths of that sequence (Moffat & Katajainen, in place, as huff_build does);
//   3. depths above 16 become 16; while the Kraft sum exceeds 1, one leaf leaves length 16 and takes the place of the deepest leaf
//      above it, which moves down one level beside it (num[16]--, num[i]--, num[i + 1] += 2 for the greatest i < 16 with num[i] > 0):
//      each step restores 2^-16 (jpeg_opt_lengths);
//   4. lengths go to the leaves by rank, the longest to the rarest: the reserved leaf holds one code of the greatest length, and is
//      dropped -- so the Kraft sum is at most 1 - 2^-16 and no code is all ones (T.81 C.2) (jpeg_opt_length_of_rank);
//   5. canonical codes, most significant bit first: lengths ascending, symbols of one length in ascending symbol order
//      (jpeg_opt_pos); the DHT segment lists the symbols in that order (jpeg_opt_dht_head).
// The decision (jpeg_opt_decide): with S = sum count x length over the four tables and V = the scan's value bits (a DC symbol carries
// `symbol` of them, an AC symbol `symbol & 15`), the picture's tables go out iff
//   header + ceil((S_own + V) / 8)  <  623 + ceil((S_annexK + V) / 8),   header = 177 + sum (21 + used symbols) + 14.
// Both sides lack the same 2 bytes of EOI and their own 0xFF00 stuffing, which depends on where the codes fall and is not counted.
#pragma once
#include <stdint.h>

#include "fl_jpeg_tables.h"

#if defined(__HIPCC__)
#define FL_JOPT_HD __host__ __device__ inline
#else
#define FL_JOPT_HD inline
#endif

namespace fl {

constexpr uint32_t kJpegOptLimit = 16;          // the longest code T.81 allows
constexpr uint32_t kJpegOptPrefixBytes = 177;   // SOI, APP0, SOF0 and the two DQT segments: the head of the cached header block
constexpr uint32_t kJpegOptSosBytes = 14;       // the SOS segment, the header block's last bytes
constexpr uint32_t kJpegOptDhtHead = 21;        // marker, length, class / destination, 16 counts
constexpr uint32_t kJpegOptMaxLeaves = 257;     // 256 symbols and the reserved leaf
static_assert(kJpegOptPrefixBytes + 4u * kJpegOptDhtHead + 2u * 12u + 2u * 162u + kJpegOptSosBytes == kJpegHeaderBytes, "the Annex K header");

// What step 3 leaves of one table: codes per length, and each length's first code and first place in the DHT's symbol list.
struct JpegOptCode {
    uint32_t num[34];
    uint32_t first_code[kJpegOptLimit + 1u], first_idx[kJpegOptLimit + 1u];
};

// Step 1: (count a, symbol a) sorts in front of (count b, symbol b)
FL_JOPT_HD bool jpeg_opt_before(uint32_t ca, uint32_t sa, uint32_t cb, uint32_t sb) { return ca < cb || (ca == cb && sa < sb); }

// Step 1 for one symbol: how many used symbols sort in front of s (meaningful where cnt[s] > 0); *used = the table's used symbols
FL_JOPT_HD uint32_t jpeg_opt_rank(const uint32_t *cnt, uint32_t s, uint32_t *used)
{
    const uint32_t cs = cnt[s];
    uint32_t r = 0, n = 0;
    for (uint32_t t = 0; t < 256u; ++t) {
        const uint32_t ct = cnt[t];
        if (ct) { ++n; r += jpeg_opt_before(ct, t, cs, s) ? 1u : 0u; }
    }
    *used = n;
    return r;
}

// Steps 2-4 for one table.  A[0 .. n): the leaves' counts in step 1's order, n >= 2 (A[0] = 1, the reserved leaf); destroyed.
// Out: c.num[1 .. 16] without the reserved leaf's code, first_code and first_idx.
FL_JOPT_HD void jpeg_opt_lengths(uint32_t *A, int n, JpegOptCode &c)
{
    uint32_t *num = c.num;
    const uint32_t limit = kJpegOptLimit;
    for (int i = 0; i < 34; ++i) num[i] = 0;
    for (uint32_t l = 0; l <= limit; ++l) c.first_code[l] = c.first_idx[l] = 0;
    if (n < 2) return;                                    // no symbol (no scan leaves a table empty): an empty DHT
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1u;
    int avbl = 1, used = 0, dpth = 0, next = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
        while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used; ++dpth; used = 0;
    }
    for (int i = 0; i < n; ++i) num[A[i] < 33u ? A[i] : 33u]++;
    for (uint32_t i = limit + 1u; i < 34u; ++i) { num[limit] += num[i]; num[i] = 0; }
    uint32_t total = 0;
    for (uint32_t i = limit; i > 0u; --i) total += num[i] << (limit - i);
    while (total > (1u << limit)) {
        num[limit]--;
        for (uint32_t i = limit - 1u; i > 0u; --i)
            if (num[i]) { num[i]--; num[i + 1u] += 2u; break; }
        total--;
    }
    for (uint32_t i = limit; i > 0u; --i)
        if (num[i]) { num[i]--; break; }                  // the reserved leaf: one code of the greatest length
    uint32_t code = 0, k = 0;
    for (uint32_t l = 1; l <= limit; ++l) {
        c.first_code[l] = code; c.first_idx[l] = k;
        code = (code + num[l]) << 1; k += num[l];
    }
    c.first_code[0] = c.first_idx[0] = 0;
}

// Step 4: the length of the used symbol of rank r (0 = the rarest)
FL_JOPT_HD uint32_t jpeg_opt_length_of_rank(const uint32_t *num, uint32_t r)
{
    uint32_t acc = 0;
    for (uint32_t l = kJpegOptLimit; l > 1u; --l) {
        acc += num[l];
        if (r < acc) return l;
    }
    return 1u;
}

// Step 5: the place of symbol s among the symbols of its length (len[s] > 0)
FL_JOPT_HD uint32_t jpeg_opt_pos(const uint8_t *len, uint32_t s)
{
    const uint32_t l = len[s];
    uint32_t p = 0;
    for (uint32_t t = 0; t < s; ++t) p += len[t] == l ? 1u : 0u;
    return p;
}

// Byte i (< kJpegOptDhtHead) of table t's DHT segment, which lists `used` symbols
FL_JOPT_HD uint8_t jpeg_opt_dht_head(uint32_t t, uint32_t i, const uint32_t *num, uint32_t used)
{
    const uint32_t lh = 2u + 1u + 16u + used;
    return i == 0u ? 0xFFu : i == 1u ? 0xC4u : i == 2u ? (uint8_t)(lh >> 8) : i == 3u ? (uint8_t)lh
         : i == 4u ? (uint8_t)(((t & 1u) << 4) | (t >> 1)) : (uint8_t)num[i - 4u];
}

FL_JOPT_HD uint32_t jpeg_opt_header_bytes(const uint32_t used[4])
{
    return kJpegOptPrefixBytes + 4u * kJpegOptDhtHead + used[0] + used[1] + used[2] + used[3] + kJpegOptSosBytes;
}

// value bits a symbol of table t carries
FL_JOPT_HD uint32_t jpeg_opt_value_bits(uint32_t t, uint32_t s) { return (t & 1u) ? (s & 15u) : s; }

FL_JOPT_HD bool jpeg_opt_decide(uint32_t header, uint64_t own_bits, uint64_t std_bits, uint64_t value_bits, bool fallback)
{
    // (a header beyond Annex K's would need a symbol Annex K lacks, which no 8-bit picture codes; the record has no room for it)
    return !fallback && header <= kJpegHeaderBytes && header + ((own_bits + value_bits + 7u) >> 3) < kJpegHeaderBytes + ((std_bits + value_bits + 7u) >> 3);
}

// Annex K's code length of every symbol of the four tables (0: the table has no such symbol)
struct JpegStdLens { uint8_t l[4][256]; };
constexpr JpegStdLens jpeg_std_lens()
{
    JpegStdLens t{};
    const HuffSpec *specs[4] = {&kDcLuma, &kAcLuma, &kDcChroma, &kAcChroma};
    for (int k = 0; k < 4; ++k)
        for (int l = 1, i = 0; l <= 16; ++l)
            for (int j = 0; j < specs[k]->len[l - 1]; ++j, ++i) t.l[k][specs[k]->val[i]] = (uint8_t)l;
    return t;
}

// The whole rule in plain loops, for the host (flgpu_debug_jpeg_optimize_tables, tests/jpeg_opt_host.cpp): counts[4][256] -> luts[4][256]
// (length << 16 | code), the four DHT segments (dht[4 * (21 + 256)], *dht_bytes) and the decision (1 / 0); -1: a table's counts sum to
// 2^32 - 1 or more.  jpeg_opt_tables_kernel spreads the same functions over a workgroup.
inline int jpeg_opt_tables_serial(const uint32_t *counts, bool fallback, uint32_t *luts, uint8_t *dht, uint32_t *dht_bytes)
{
    constexpr JpegStdLens std_lens = jpeg_std_lens();
    uint32_t used[4], at = 0;
    uint64_t own = 0, std_bits = 0, val = 0;
    for (uint32_t t = 0; t < 4u; ++t) {
        const uint32_t *cnt = counts + 256u * t;
        uint32_t A[kJpegOptMaxLeaves + 1u], rank[256];
        uint8_t len[256], vals[256];
        JpegOptCode code;
        uint64_t sum = 0;
        for (uint32_t s = 0; s < 256u; ++s) sum += cnt[s];
        if (sum >= 0xffffffffull) return -1;
        A[0] = 1u;
        used[t] = 0;
        for (uint32_t s = 0; s < 256u; ++s) {
            rank[s] = jpeg_opt_rank(cnt, s, &used[t]);
            if (cnt[s]) A[1u + rank[s]] = cnt[s];
        }
        jpeg_opt_lengths(A, (int)used[t] + 1, code);
        for (uint32_t s = 0; s < 256u; ++s) len[s] = cnt[s] ? (uint8_t)jpeg_opt_length_of_rank(code.num, rank[s]) : (uint8_t)0;
        for (uint32_t s = 0; s < 256u; ++s) {
            luts[256u * t + s] = 0u;
            if (!len[s]) continue;
            const uint32_t pos = jpeg_opt_pos(len, s);
            luts[256u * t + s] = ((uint32_t)len[s] << 16) | (code.first_code[len[s]] + pos);
            vals[code.first_idx[len[s]] + pos] = (uint8_t)s;
            own += (uint64_t)cnt[s] * len[s];
            std_bits += (uint64_t)cnt[s] * std_lens.l[t][s];
            val += (uint64_t)cnt[s] * jpeg_opt_value_bits(t, s);
        }
        for (uint32_t i = 0; i < kJpegOptDhtHead; ++i) dht[at + i] = jpeg_opt_dht_head(t, i, code.num, used[t]);
        for (uint32_t i = 0; i < used[t]; ++i) dht[at + kJpegOptDhtHead + i] = vals[i];
        at += kJpegOptDhtHead + used[t];
    }
    *dht_bytes = at;
    return jpeg_opt_decide(jpeg_opt_header_bytes(used), own, std_bits, val, fallback) ? 1 : 0;
}

} // namespace fl
