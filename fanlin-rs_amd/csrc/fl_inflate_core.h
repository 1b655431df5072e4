// fl_inflate_core.h -- everything data-dependent of the device inflate (fl_inflate.hip), as code that compiles for the host and for
// the device: the canonical table build, one token step, the walk over a subsequence, the readiness rule of the write-and-resolve
// loop and the Adler-32 combine.  The kernel runs these per thread between barriers; the host twin (png_inflate_model,
// fl_pngsrc.cpp) runs the same functions in plain loops over arrays of the kernel's LDS sizes, so an index that leaves an array on
// the device leaves it under the sanitizers on the CPU.  Plain C++, no HIP needed.
//
// Positions are bit positions.  `win` is a window of 32-bit words of the stream (the payload itself, or a strip's copy in LDS); a read
// past its `nwords` gives zero bits, and every token is held against `limit`, the first bit that is not the stream's.
#pragma once
#include <stdint.h>

#include "fl_inflate.h"

#if defined(__HIPCC__)
#define FL_INF_HD __host__ __device__ inline
#else
#define FL_INF_HD inline
#endif

namespace fl {

constexpr uint32_t kInfStripBits = kInfSubBits * kInfSubs;
constexpr uint32_t kInfMaxTokenBits = 15 + 5 + 15 + 13; // a length code and its extra bits, a distance code and its extra bits
// the strip's words, one more for a start that is not word-aligned, and what a 64-bit read at the last token's first bit touches
constexpr uint32_t kInfWindowWords = kInfStripBits / 32u + 1u + 3u;
constexpr uint32_t kInfHeaderWords = 160; // a dynamic block's header: at most 17 + 19 x 3 + 316 x 14 = 4,498 bits
constexpr uint32_t kInfFastBits = 10;

// states of a subsequence: the bit at which the first token behind it begins, or ...
constexpr uint32_t kInfEob = 0x80000000u;     // ... | the bit behind the end-of-block symbol it met
constexpr uint32_t kInfInvalid = 0x40000000u; // an invalid code, or a token that runs past the stream
constexpr uint32_t kInfDead = 0x20000000u;    // lies behind the block's end (or behind an invalid token)
constexpr uint32_t kInfFlags = kInfEob | kInfInvalid | kInfDead;
constexpr uint32_t kInfNever = 0xffffffffu;   // no state a walk ever stores

constexpr uint32_t kAdlerMod = 65521u;

struct InfTable {
    uint16_t fast[1u << kInfFastBits]; // (symbol << 4) | length, 0 = a longer code (or none)
    uint16_t count[16];
    uint16_t symbol[288];
    uint32_t max_len;
};

// 64 bits of the stream from `bit` on
FL_INF_HD uint64_t inf_peek(const uint32_t *win, uint64_t nwords, uint64_t bit)
{
    const uint64_t i = bit >> 5;
    const uint32_t s = (uint32_t)bit & 31u;
    const uint64_t w0 = i < nwords ? win[i] : 0u, w1 = i + 1u < nwords ? win[i + 1u] : 0u, w2 = i + 2u < nwords ? win[i + 2u] : 0u;
    uint64_t v = (w1 << 32 | w0) >> s;
    if (s) v |= w2 << (64u - s);
    return v;
}

// Canonical code from lengths (RFC 1951 3.2.2), lengths at most 15 and nsym at most 288.  false: over-subscribed, or incomplete with
// more than one code -- the rule of the host inflate, so both accept the same headers.
FL_INF_HD bool inf_build(InfTable &h, const uint8_t *len, uint32_t nsym)
{
    if (nsym > 288u) return false;
    for (uint32_t l = 0; l < 16; ++l) h.count[l] = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
        if (len[s] > 15u) return false;
        h.count[len[s]]++;
    }
    for (uint32_t v = 0; v < (1u << kInfFastBits); ++v) h.fast[v] = 0;
    h.max_len = 0;
    if (h.count[0] == nsym) return true; // no codes at all: decoding any symbol fails
    int left = 1;
    for (uint32_t l = 1; l < 16; ++l) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return false;
        if (h.count[l]) h.max_len = l;
    }
    if (left > 0 && nsym - h.count[0] != 1u) return false;
    uint16_t offs[16];
    offs[0] = 0; offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (uint32_t s = 0; s < nsym; ++s)
        if (len[s]) {
            const uint32_t at = offs[len[s]]++;
            if (at < 288u) h.symbol[at] = (uint16_t)s;
        }
    // fast table: every code of up to kInfFastBits bits, bit-reversed (codes are packed starting from their top bit)
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= kInfFastBits; ++l) {
        for (uint32_t k = 0; k < h.count[l]; ++k, ++code, ++idx) {
            uint32_t rev = 0;
            for (uint32_t b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1u - b);
            if (idx >= 288u) return false;
            const uint16_t e = (uint16_t)(h.symbol[idx] << 4 | l);
            for (uint32_t v = rev; v < (1u << kInfFastBits); v += 1u << l) h.fast[v] = e;
        }
        code <<= 1;
    }
    return true;
}

// One symbol from the low bits of v: >= 0 and `used` bits, or -1 (no such code).
FL_INF_HD int inf_symbol(const InfTable &h, uint64_t v, uint32_t &used)
{
    const uint16_t e = h.fast[v & ((1u << kInfFastBits) - 1u)];
    if (e) { used = e & 15u; return e >> 4; }
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= h.max_len && l < 16u; ++l) {
        code |= (int)(v & 1u);
        v >>= 1;
        const int count = h.count[l];
        if (code - count < first) {
            const int at = index + (code - first);
            if (at < 0 || at >= 288) return -1;
            used = l;
            return h.symbol[at];
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

enum : uint32_t { kInfLiteral = 0, kInfMatch = 1, kInfEnd = 2, kInfBad = 3 };
struct InfToken {
    uint32_t kind;
    uint32_t bits; // of the whole token, at most kInfMaxTokenBits
    uint32_t len;  // output bytes: 1 for a literal, 3..258 for a match
    uint32_t val;  // the literal, or the distance 1..32768
};

// The token whose first bit is the lowest of v.  Bases and extra bits of RFC 1951 3.2.5 as arithmetic: no table to index.
FL_INF_HD InfToken inf_token(const InfTable &lit, const InfTable &dist, uint64_t v)
{
    InfToken t{kInfBad, 0, 0, 0};
    uint32_t n = 0;
    int sym = inf_symbol(lit, v, n);
    if (sym < 0) return t;
    if (sym < 256) { t.kind = kInfLiteral; t.bits = n; t.len = 1; t.val = (uint32_t)sym; return t; }
    if (sym == 256) { t.kind = kInfEnd; t.bits = n; return t; }
    const uint32_t ls = (uint32_t)sym - 257u;
    if (ls >= 29u) return t;
    uint32_t eb = ls < 8u || ls == 28u ? 0u : (ls - 4u) >> 2;
    const uint32_t lbase = ls == 28u ? 258u : ls < 8u ? 3u + ls : 3u + ((4u + (ls & 3u)) << eb);
    const uint32_t len = lbase + (uint32_t)((v >> n) & ((1u << eb) - 1u));
    n += eb;
    uint32_t m = 0;
    const int ds = inf_symbol(dist, v >> n, m);
    if (ds < 0 || ds >= 30) return t;
    n += m;
    eb = ds < 4 ? 0u : ((uint32_t)ds - 2u) >> 1;
    const uint32_t dbase = ds < 4 ? 1u + (uint32_t)ds : 1u + ((2u + ((uint32_t)ds & 1u)) << eb);
    t.val = dbase + (uint32_t)((v >> n) & ((1u << eb) - 1u));
    n += eb;
    t.kind = kInfMatch; t.bits = n; t.len = len;
    return t;
}

// The walk over one subsequence: tokens from bit p until one begins at or behind `bound`.  Returns the state (above); out_bytes = what
// the tokens write, tokens = how many were decoded.  Every token has at least one bit, so the walk ends.
FL_INF_HD uint32_t inf_walk(const InfTable &lit, const InfTable &dist, const uint32_t *win, uint32_t nwords, uint32_t p, uint32_t bound, uint32_t limit,
                            uint32_t &out_bytes, uint32_t &tokens)
{
    out_bytes = 0; tokens = 0;
    while (p < bound) {
        const InfToken t = inf_token(lit, dist, inf_peek(win, nwords, p));
        if (t.kind == kInfBad || t.bits > limit || p > limit - t.bits) return kInfInvalid;
        ++tokens;
        p += t.bits;
        if (t.kind == kInfEnd) return p | kInfEob;
        out_bytes += t.len;
    }
    return p;
}

// The readiness rule: a match at output position o may be copied once everything below `done` is final (done = the output position
// of the first match of the strip that has not been copied yet).  A match that overlaps itself repeats the dist bytes in front of it.
FL_INF_HD bool inf_ready(uint32_t o, uint32_t len, uint32_t dist, uint32_t done)
{
    return dist >= len ? o - dist + len <= done : o <= done;
}

// a byte another wave of the workgroup wrote before the last fence + barrier: read past the vector L1 on the device
FL_INF_HD uint8_t inf_load(const uint8_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}

enum : int { kInfFinished = 0, kInfPending = 1, kInfFail = 2 };
// One thread's share of a write-and-resolve round: on through its tokens from (p, o), literals stored as it passes them, matches
// copied while they are ready.  kInfPending: stopped in front of a match that is not (p and o stay at it).  kInfFail: a distance that
// reaches before the start of the stream, or a write beyond `cap`.
FL_INF_HD int inf_resolve(const InfTable &lit, const InfTable &dist, const uint32_t *win, uint32_t nwords, uint32_t &p, uint32_t bound, uint32_t &o, uint32_t done,
                          uint8_t *out, uint32_t cap)
{
    while (p < bound) {
        const InfToken t = inf_token(lit, dist, inf_peek(win, nwords, p));
        if (t.kind == kInfBad) return kInfFail;
        if (t.kind == kInfEnd) { p = bound; return kInfFinished; }
        if (o > cap || t.len > cap - o) return kInfFail;
        if (t.kind == kInfLiteral) {
            out[o] = (uint8_t)t.val;
        } else {
            if (t.val > o) return kInfFail;
            if (!inf_ready(o, t.len, t.val, done)) return kInfPending;
            const uint8_t *from = out + (o - t.val);
            if (t.val >= t.len) for (uint32_t i = 0; i < t.len; ++i) out[o + i] = inf_load(from + i);
            else for (uint32_t i = 0, k = 0; i < t.len; ++i) { out[o + i] = inf_load(from + k); k = k + 1u == t.val ? 0u : k + 1u; }
        }
        o += t.len;
        p += t.bits;
    }
    return kInfFinished;
}

// A dynamic block's header from bit p of `win` on (behind BFINAL and BTYPE): the code-length code, the run-length coded lengths, both
// tables.  `cl` is scratch for the code-length code.  Returns the bit behind the header, or 0: damaged.
FL_INF_HD uint32_t inf_dynamic_header(const uint32_t *win, uint32_t nwords, uint32_t p, uint32_t limit, InfTable &cl, InfTable &lit, InfTable &dist, uint8_t *lengths /* [320] */)
{
    if (p > limit || limit - p < 14u) return 0;
    uint64_t v = inf_peek(win, nwords, p);
    const uint32_t nlen = (uint32_t)(v & 31u) + 257u, ndist = (uint32_t)((v >> 5) & 31u) + 1u, ncode = (uint32_t)((v >> 10) & 15u) + 4u;
    p += 14u;
    if (nlen > 286u || ndist > 30u) return 0;
    for (uint32_t k = 0; k < 320u; ++k) lengths[k] = 0;
    for (uint32_t k = 0; k < ncode; ++k) {
        if (limit - p < 3u) return 0;
        const uint32_t order = k < 3u ? 16u + k : k == 3u ? 0u : (k & 1u) ? 8u - ((k - 3u) >> 1) : 7u + ((k - 2u) >> 1);
        lengths[order] = (uint8_t)(inf_peek(win, nwords, p) & 7u);
        p += 3u;
    }
    if (!inf_build(cl, lengths, 19)) return 0;
    for (uint32_t k = 0; k < 19u; ++k) lengths[k] = 0;
    uint32_t idx = 0;
    while (idx < nlen + ndist) {
        v = inf_peek(win, nwords, p);
        uint32_t n = 0;
        const int sym = inf_symbol(cl, v, n);
        if (sym < 0 || limit - p < n) return 0;
        p += n; v >>= n;
        if (sym < 16) { lengths[idx++] = (uint8_t)sym; continue; }
        uint32_t rep, val = 0, eb;
        if (sym == 16) {
            if (idx == 0) return 0;
            val = lengths[idx - 1u]; eb = 2; rep = 3u + (uint32_t)(v & 3u);
        } else if (sym == 17) { eb = 3; rep = 3u + (uint32_t)(v & 7u); }
        else { eb = 7; rep = 11u + (uint32_t)(v & 127u); }
        if (limit - p < eb) return 0;
        p += eb;
        if (idx + rep > nlen + ndist) return 0;
        while (rep--) lengths[idx++] = (uint8_t)val;
    }
    if (lengths[256] == 0) return 0; // no end-of-block code
    if (!inf_build(lit, lengths, nlen) || !inf_build(dist, lengths + nlen, ndist)) return 0;
    return p;
}

// The fixed code's two tables (RFC 1951 3.2.6); `lengths` is scratch of 288 bytes.
FL_INF_HD void inf_fixed_tables(InfTable &lit, InfTable &dist, uint8_t *lengths)
{
    for (uint32_t s = 0; s < 288u; ++s) lengths[s] = s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8;
    inf_build(lit, lengths, 288);
    for (uint32_t s = 0; s < 32u; ++s) lengths[s] = 5; // (codes 30 and 31 exist in the fixed code and are invalid in a stream)
    inf_build(dist, lengths, 32);
}

// Adler-32 by pieces.  A piece of 16 bytes at offset j of n bytes adds sum(d_i) to a and sum((n - j - i) d_i) to b: that is the
// combine rule for concatenation, b(A | B) = b(A) + b(B) + len(B) (a(A) - 1), written out per piece, so pieces may be summed in any
// order.  s1 / s2 are one thread's running sums; w = (n - j) mod 65521.
FL_INF_HD void inf_adler_piece(uint64_t &s1, uint64_t &s2, const uint8_t *d, uint32_t k, uint32_t w)
{
    uint32_t s = 0, t = 0;
    for (uint32_t i = 0; i < k; ++i) { s += d[i]; t += i * d[i]; }
    s1 += s;
    s2 += (uint64_t)w * s + (uint64_t)kAdlerMod * 64u - t; // (t <= 15 x 4080 < 64 x 65521: the sum stays positive)
}
// the check value of n bytes from the sums of all pieces
FL_INF_HD uint32_t inf_adler_finish(uint64_t s1, uint64_t s2, uint64_t n)
{
    const uint32_t a = (uint32_t)((1u + s1) % kAdlerMod), b = (uint32_t)((n + s2) % kAdlerMod);
    return b << 16 | a;
}

} // namespace fl
