// fl_png.hip -- the PNG encoder on gfx950: row filters, deflate and framing, so that what leaves the GPU is the finished
// PNG file.
//
// Replaces `PngEncoder::new_with_quality(&mut buffer, ct, FilterType::Adaptive)` + `write_with_encoder` (reference
// src/handler.rs:264-273): 8-bit samples, colour type from the channel count, no interlace, the filter of every row chosen
// by the png crate's adaptive rule, a zlib stream at the effort the quality maps to.  Byte identity with the crate's deflate
// is not a goal; the pixels a decoder gets back are identical.
//
// Three launches per batch; inside a launch no workgroup waits on another:
//   png_filter_kernel    one wave per row: the four candidate filters (Sub, Up, Average, Paeth) in registers, their scores
//                        reduced across the wave, the lowest (the later one on a tie) written with its filter byte.
//   png_deflate_kernel   one workgroup per 32 KB segment of a picture's filtered stream.  The segment and the 32 KB in front
//                        of it are staged in LDS; hash chains are linked in rounds of 256 positions (a position links to
//                        the last one of an EARLIER round with its 3-byte hash: the head table is raised with atomicMax, so
//                        the links do not depend on the order of the atomics), or to the last one in its own wave (twelve
//                        ballots); each lane of the first wave parses 512 bytes (greedy, or lazy
//                        by one position), histograms go up by LDS atomics; one lane builds each length-limited Huffman code
//                        (15 / 15 / 7 bits) and the block header; every lane measures its symbols' bits, an exclusive scan
//                        places them, and they are ORed into an LDS bit buffer.  A segment that would not shrink is one
//                        stored block.  Non-final segments end with an empty stored block, so each is whole bytes and one
//                        IDAT chunk; its CRC-32 is per-lane slices shifted into place (crc32_combine's x^(8n) mod P) and
//                        XOR-reduced; its Adler-32 partial sums (A, B) go to a record.
//   png_frame_kernel     one workgroup per picture: signature, IHDR, the segments' chunks in order, an IDAT holding the
//                        combined Adler-32, IEND; the length (or 0 if the file does not fit dst_cap) into the result word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_huff_build.h"
#include "fl_png.h"
#include "fl_types.h"
#include "fl_wave.h"

namespace fl {

namespace {

// ---------------------------------------------------------------- CRC-32 tables (reflected, polynomial 0xEDB88320) --

constexpr uint32_t kCrcPoly = 0xedb88320u;

// a(x) * b(x) modulo P(x), reflected bit order (zlib's multmodp), in a fixed 32 steps
constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

struct CrcTables {
    uint32_t byte[256];  // the usual byte-at-a-time table
    uint32_t x2n[32];    // x^(2^k) mod P
};

constexpr CrcTables make_crc_tables()
{
    CrcTables t{};
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t v = n;
        for (int k = 0; k < 8; ++k) v = (v & 1u) ? (v >> 1) ^ kCrcPoly : v >> 1;
        t.byte[n] = v;
    }
    uint32_t p = 1u << 30; // x^1
    t.x2n[0] = p;
    for (int k = 1; k < 32; ++k) t.x2n[k] = p = crc_mulmod(p, p);
    return t;
}

__constant__ CrcTables kCrc = make_crc_tables();

// x^(8 n) mod P: what n zero bytes do to a CRC register
__device__ __forceinline__ uint32_t crc_shift_op(uint32_t n)
{
    uint32_t p = 1u << 31, k = 3;
    while (n) {
        if (n & 1u) p = crc_mulmod(kCrc.x2n[k & 31u], p);
        n >>= 1;
        ++k;
    }
    return p;
}

__device__ __forceinline__ uint32_t crc_bytes(uint32_t r, const uint8_t *b, uint32_t n) // raw register update (no conditioning)
{
    for (uint32_t i = 0; i < n; ++i) r = kCrc.byte[(r ^ b[i]) & 255u] ^ (r >> 8);
    return r;
}

__device__ __forceinline__ void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// ---------------------------------------------------------------- wave / workgroup helpers (256 threads) --

__device__ __forceinline__ uint64_t wg_sum64(uint64_t v, uint64_t *s)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) s[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t t = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPngThreads / 64u; ++i) t += s[i];
    return t;
}

// ---------------------------------------------------------------- kernel 1: row filters --

__device__ __forceinline__ int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint32_t filt_byte(uint32_t f, int x, int a, int b, int c)
{
    const int pred = f == 1u ? a : f == 2u ? b : f == 3u ? ((a + b) >> 1) : paeth(a, b, c);
    return (uint32_t)(x - pred) & 255u;
}

__global__ __launch_bounds__(kPngThreads) void png_filter_kernel(const PngJob *__restrict__ jobs, uint32_t njobs, uint32_t total_rows)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * (kPngThreads / 64u) + (threadIdx.x >> 6);
    if (r >= total_rows) return;
    const PngJob &jb = jobs[find_first_le(jobs, njobs, r, &PngJob::row0)];
    const uint32_t y = r - jb.row0, bpp = jb.c;
    const size_t rb = (size_t)jb.w * jb.c;
    const uint8_t *cur = jb.src + (size_t)y * rb;
    const uint8_t *up = cur - rb; // read only when y > 0
    // png 0.17 filter() with AdaptiveFilterType::Adaptive: Sub, Up, Avg, Paeth in that order, score sum |(i8)byte|, `<=`
    uint64_t s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (size_t x = lane; x < rb; x += 64u) {
        const int v = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = y ? up[x] : 0, c = (y && x >= bpp) ? up[x - bpp] : 0;
        s1 += (uint32_t)abs((int)(int8_t)filt_byte(1u, v, a, b, c));
        s2 += (uint32_t)abs((int)(int8_t)filt_byte(2u, v, a, b, c));
        s3 += (uint32_t)abs((int)(int8_t)filt_byte(3u, v, a, b, c));
        s4 += (uint32_t)abs((int)(int8_t)filt_byte(4u, v, a, b, c));
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4);
    uint32_t f = 1u;
    uint64_t best = s1;
    if (s2 <= best) { best = s2; f = 2u; }
    if (s3 <= best) { best = s3; f = 3u; }
    if (s4 <= best) { best = s4; f = 4u; }
    uint8_t *out = jb.filt + (size_t)y * (rb + 1u);
    if (lane == 0u) out[0] = (uint8_t)f;
    for (size_t x = lane; x < rb; x += 64u) {
        const int v = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = y ? up[x] : 0, c = (y && x >= bpp) ? up[x - bpp] : 0;
        out[1u + x] = (uint8_t)filt_byte(f, v, a, b, c);
    }
}

// ---------------------------------------------------------------- kernel 2: deflate one segment --

// The parse runs on the first wave: each of its lanes takes 512 bytes.  (128 bytes on all four waves clip matches so often that
// flat and line-art pictures come out four times longer than zlib's: a run costs one length-<=128 match per lane.)
constexpr uint32_t kLaneBytes = kPngSegBytes / 64u;
constexpr uint32_t kHashBits = 12;
constexpr uint32_t kWinBytes = 2u * kPngSegBytes;
// LDS: window (later the output bit buffer) | chain links (later the CRC table) | head table (later histograms and codes) | misc
constexpr uint32_t kLdsPrev = kWinBytes, kLdsHead = kLdsPrev + 2u * kPngSegBytes, kLdsMisc = kLdsHead + (4u << kHashBits);
constexpr uint32_t kDeflateLds = kLdsMisc + 4096u;
// head-region words once the chains are linked
constexpr uint32_t kHistLit = 0, kHistDist = 288, kHistCl = 320, kCodeLit = 352, kCodeDist = 640, kCodeCl = 672, kKeyL = 704,
                   kSymL = 992, kKeyD = 1280, kSymD = 1312, kKeyC = 1344, kSymC = 1364, kRle = 1400, kLens = 1720, kHeadWordsUsed = 2040;
static_assert(kHeadWordsUsed * 4u <= (4u << kHashBits), "head region");
// misc-region words
constexpr uint32_t kMiscScan = 0, kMiscRed = 8, kMiscHdrBits = 24, kMiscHlit = 25, kMiscHdist = 26, kMiscHclen = 27, kMiscNrle = 28,
                   kMiscBuild0 = 64, kMiscBuild1 = 160;

__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Level { uint32_t depth, nice, lazy; };
__constant__ Level kLevels[3] = {{8u, 64u, 0u}, {64u, 128u, 1u}, {256u, 258u, 1u}}; // Fast, Default, Best

__device__ __forceinline__ uint32_t hash3(const uint8_t *w, uint32_t p)
{
    const uint32_t v = (uint32_t)w[p] | ((uint32_t)w[p + 1u] << 8) | ((uint32_t)w[p + 2u] << 16);
    return (v * 2654435761u) >> (32u - kHashBits);
}

__device__ __forceinline__ uint32_t len_code(uint32_t len, uint32_t *eb, uint32_t *ev)
{
    if (len == 258u) { *eb = 0; *ev = 0; return 285u; }
    const uint32_t l = len - 3u;
    if (l < 8u) { *eb = 0; *ev = 0; return 257u + l; }
    const uint32_t nb = 31u - (uint32_t)__clz(l);
    *eb = nb - 2u; *ev = l & ((1u << (nb - 2u)) - 1u);
    return 257u + 4u * (nb - 1u) + ((l >> (nb - 2u)) & 3u);
}

__device__ __forceinline__ uint32_t dist_code(uint32_t dist, uint32_t *eb, uint32_t *ev)
{
    const uint32_t x = dist - 1u;
    if (x < 4u) { *eb = 0; *ev = 0; return x; }
    const uint32_t nb = 31u - (uint32_t)__clz(x);
    *eb = nb - 1u; *ev = x & ((1u << (nb - 1u)) - 1u);
    return 2u * nb + ((x >> (nb - 1u)) & 1u);
}

// longest match for window position p among its chain, not reaching past hi
__device__ __forceinline__ uint32_t find_match(const uint8_t *win, const uint16_t *prev, uint32_t H, uint32_t p, uint32_t hi,
                                               uint32_t depth, uint32_t nice, uint32_t *bdist)
{
    const uint32_t maxlen = min(258u, hi - p);
    *bdist = 0;
    if (maxlen < 3u) return 0;
    uint32_t d = prev[p - H], q = p - d, best = 2u;
    for (uint32_t k = 0; d && k < depth; ++k) {
        const uint32_t dist = p - q;
        if (dist > 32768u) break;
        if (win[q + best] == win[p + best]) {
            uint32_t l = 0;
            while (l < maxlen && win[q + l] == win[p + l]) ++l;
            if (l > best) {
                best = l; *bdist = dist;
                if (l >= nice || l == maxlen) break;
            }
        }
        if (q < H) break; // history positions carry no link of their own
        d = prev[q - H];
        q -= d;
    }
    return best >= 3u ? best : 0u;
}

__device__ __forceinline__ void put_bits(uint32_t *buf, uint32_t pos, uint32_t val, uint32_t n)
{
    if (!n) return;
    const uint32_t w = pos >> 5, sh = pos & 31u;
    atomicOr(&buf[w], val << sh);
    if (sh + n > 32u) atomicOr(&buf[w + 1u], val >> (32u - sh));
}

__global__ __launch_bounds__(kPngThreads) void png_deflate_kernel(const PngJob *__restrict__ jobs, uint32_t njobs)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];
    const uint32_t tid = threadIdx.x, g = blockIdx.x;
    const PngJob &jb = jobs[find_first_le(jobs, njobs, g, &PngJob::seg0)];
    const uint32_t s = g - jb.seg0;
    const uint64_t seg_start = (uint64_t)s * kPngSegBytes;
    const uint32_t L = (uint32_t)min<uint64_t>(kPngSegBytes, jb.fbytes - seg_start);
    const uint32_t H = s ? kPngSegBytes : 0u, N = H + L;
    const bool first = s == 0u, final = s + 1u == jb.nseg;
    const Level lv = kLevels[min(jb.level, 2u)];
    uint8_t *win = png_lds;
    uint16_t *prev = reinterpret_cast<uint16_t *>(png_lds + kLdsPrev);
    uint32_t *head = reinterpret_cast<uint32_t *>(png_lds + kLdsHead);
    uint32_t *misc = reinterpret_cast<uint32_t *>(png_lds + kLdsMisc);
    uint64_t *red = reinterpret_cast<uint64_t *>(misc + kMiscRed);

    // ---- stage history + segment (16-byte pieces: the scratch is 256-byte aligned and padded to 256 bytes) ----
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(jb.filt + seg_start - H);
        uint4 *dst = reinterpret_cast<uint4 *>(win);
        for (uint32_t i = tid; i < (N + 15u) / 16u; i += kPngThreads) dst[i] = src[i];
    }
    for (uint32_t i = tid; i < (1u << kHashBits); i += kPngThreads) head[i] = 0u;
    __syncthreads();
    const uint32_t lo = min(H + tid * kLaneBytes, N), hi = min(lo + kLaneBytes, N); // (lanes of waves 1-3: empty ranges)
    // ---- Adler-32 partial sums of the segment: A = sum b, B = sum (L - k) b ----
    uint64_t pa = 0, pb = 0;
    for (uint32_t p = lo; p < hi; ++p) { const uint32_t b = win[p]; pa += b; pb += (uint64_t)(N - p) * b; }
    const uint64_t adler_a = wg_sum64(pa, red) % 65521u;
    const uint64_t adler_b = wg_sum64(pb, red) % 65521u;

    // ---- hash chains: rounds of 256 positions; a position links to the last one with its hash in its own wave (twelve
    // ballots find the lanes whose hash equals this lane's), else to the last one of an earlier round ----
    const uint32_t nh = N >= 3u ? N - 2u : 0u;
    const uint32_t lane = tid & 63u;
    for (uint32_t base = 0; base < nh; base += kPngThreads) {
        const uint32_t p = base + tid;
        const bool valid = p < nh;
        const uint32_t h = valid ? hash3(win, p) : 0u;
        uint64_t same = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < kHashBits; ++b) {
            const uint64_t bal = __ballot(valid && ((h >> b) & 1u));
            same &= ((h >> b) & 1u) ? bal : ~bal;
        }
        const uint64_t below = same & ((1ull << lane) - 1ull);
        if (valid && p >= H) {
            uint32_t d;
            if (below) d = lane - (63u - (uint32_t)__clzll(below));
            else { const uint32_t q1 = head[h]; d = q1 ? p - (q1 - 1u) : 0u; }
            prev[p - H] = (uint16_t)(d <= 32768u ? d : 0u);
        }
        __syncthreads();
        if (valid) atomicMax(&head[h], p + 1u);
        __syncthreads();
    }
    for (uint32_t p = max(nh, H) + tid; p < N; p += kPngThreads) prev[p - H] = 0; // the last two positions: no 3-byte hash
    for (uint32_t i = tid; i < kHeadWordsUsed; i += kPngThreads) head[i] = 0u;
    __syncthreads();

    // ---- parse this lane's 128 bytes; symbols to scratch, histograms by LDS atomics ----
    uint32_t *hl = head + kHistLit, *hd = head + kHistDist;
    uint16_t *sym = jb.syms + (size_t)s * kPngSegBytes + (size_t)min(tid, 63u) * kLaneBytes;
    uint32_t ns = 0;
    {
        uint32_t p = lo, ml = 0, md = 0;
        bool have = false;
        while (p < hi) {
            if (!have) ml = find_match(win, prev, H, p, hi, lv.depth, lv.nice, &md);
            have = false;
            if (ml >= 3u && lv.lazy && ml < lv.nice && p + 1u < hi) {
                uint32_t d2;
                const uint32_t l2 = find_match(win, prev, H, p + 1u, hi, lv.depth, lv.nice, &d2);
                if (l2 > ml) {
                    sym[ns++] = win[p]; atomicAdd(&hl[win[p]], 1u);
                    ++p; ml = l2; md = d2; have = true;
                    continue;
                }
            }
            if (ml >= 3u) {
                uint32_t eb, ev;
                sym[ns++] = (uint16_t)(256u + ml - 3u);
                sym[ns++] = (uint16_t)(md - 1u);
                atomicAdd(&hl[len_code(ml, &eb, &ev)], 1u);
                atomicAdd(&hd[dist_code(md, &eb, &ev)], 1u);
                p += ml;
            } else {
                sym[ns++] = win[p]; atomicAdd(&hl[win[p]], 1u);
                ++p;
            }
        }
    }
    __syncthreads();
    if (tid == 0u) {
        hl[256] = 1u; // end of block
        // every code gets at least two symbols (a one-symbol code is incomplete, which inflate refuses for the lengths code)
        uint32_t used = 0;
        for (uint32_t k = 0; k < 286u; ++k) used += hl[k] ? 1u : 0u;
        for (uint32_t k = 0; k < 286u && used < 2u; ++k) if (!hl[k]) { hl[k] = 1u; ++used; }
        used = 0;
        for (uint32_t k = 0; k < 30u; ++k) used += hd[k] ? 1u : 0u;
        for (uint32_t k = 0; k < 30u && used < 2u; ++k) if (!hd[k]) { hd[k] = 1u; ++used; }
    }
    __syncthreads();
    // ---- rank the used symbols by (count, symbol) ----
    for (uint32_t i = tid; i < 286u + 30u; i += kPngThreads) {
        const bool lit = i < 286u;
        const uint32_t *hist = lit ? hl : hd, n = lit ? 286u : 30u, sy = lit ? i : i - 286u, f = hist[sy];
        if (!f) continue;
        uint32_t rank = 0;
        for (uint32_t t = 0; t < n; ++t) { const uint32_t ft = hist[t]; rank += (ft && (ft < f || (ft == f && t < sy))) ? 1u : 0u; }
        (lit ? head + kKeyL : head + kKeyD)[rank] = f;
        (lit ? head + kSymL : head + kSymD)[rank] = sy;
    }
    __syncthreads();
    if (tid == 0u || tid == 64u) { // two waves build the two codes side by side
        const bool lit = tid == 0u;
        const uint32_t *hist = lit ? hl : hd, n = lit ? 286u : 30u;
        int used = 0;
        for (uint32_t t = 0; t < n; ++t) used += hist[t] ? 1 : 0;
        huff_build(head + (lit ? kKeyL : kKeyD), head + (lit ? kSymL : kSymD), used, 15u, n, head + (lit ? kCodeLit : kCodeDist),
                   misc + (lit ? kMiscBuild0 : kMiscBuild1));
    }
    __syncthreads();
    const uint32_t *cl = head + kCodeLit, *cd = head + kCodeDist, *cc = head + kCodeCl;
    if (tid == 0u) {
        // block header: the two codes' lengths as one run-length coded sequence (RFC 1951 3.2.7)
        uint32_t hlit = 257, hdist = 1;
        for (uint32_t k = 0; k < 286u; ++k) if (cl[k]) hlit = max(hlit, k + 1u);
        for (uint32_t k = 0; k < 30u; ++k) if (cd[k]) hdist = max(hdist, k + 1u);
        uint32_t *lens = head + kLens, *rle = head + kRle, *hc = head + kHistCl;
        const uint32_t total = hlit + hdist;
        for (uint32_t k = 0; k < total; ++k) lens[k] = (k < hlit ? cl[k] : cd[k - hlit]) >> 16;
        uint32_t nr = 0;
        for (uint32_t i = 0; i < total;) {
            const uint32_t v = lens[i];
            uint32_t run = 1;
            while (i + run < total && lens[i + run] == v) ++run;
            uint32_t r = run;
            if (v == 0u) {
                while (r >= 11u) { const uint32_t m = min(r, 138u); rle[nr++] = 18u | ((m - 11u) << 8); hc[18]++; r -= m; }
                if (r >= 3u) { rle[nr++] = 17u | ((r - 3u) << 8); hc[17]++; r = 0; }
            } else {
                rle[nr++] = v; hc[v]++; --r;
                while (r >= 3u) { const uint32_t m = min(r, 6u); rle[nr++] = 16u | ((m - 3u) << 8); hc[16]++; r -= m; }
            }
            while (r > 0u) { rle[nr++] = v; hc[v]++; --r; }
            i += run;
        }
        uint32_t used = 0;
        for (uint32_t k = 0; k < 19u; ++k) used += hc[k] ? 1u : 0u;
        for (uint32_t k = 0; k < 19u && used < 2u; ++k) if (!hc[k]) { hc[k] = 1u; ++used; }
        uint32_t *key = head + kKeyC, *sy = head + kSymC;
        for (uint32_t a = 0; a < 19u; ++a) {
            if (!hc[a]) continue;
            uint32_t rank = 0;
            for (uint32_t t = 0; t < 19u; ++t) rank += (hc[t] && (hc[t] < hc[a] || (hc[t] == hc[a] && t < a))) ? 1u : 0u;
            key[rank] = hc[a]; sy[rank] = a;
        }
        huff_build(key, sy, (int)used, 7u, 19u, head + kCodeCl, misc + kMiscBuild0);
        uint32_t hclen = 4;
        for (uint32_t k = 0; k < 19u; ++k) if (cc[kClOrder[k]]) hclen = max(hclen, k + 1u);
        uint32_t bits = 3u + 5u + 5u + 4u + 3u * hclen;
        for (uint32_t k = 0; k < nr; ++k) {
            const uint32_t a = rle[k] & 255u;
            bits += (cc[a] >> 16) + (a == 16u ? 2u : a == 17u ? 3u : a == 18u ? 7u : 0u);
        }
        misc[kMiscHdrBits] = bits; misc[kMiscHlit] = hlit; misc[kMiscHdist] = hdist; misc[kMiscHclen] = hclen; misc[kMiscNrle] = nr;
    }
    __syncthreads();
    // ---- every lane measures its symbols; an exclusive scan places them ----
    uint32_t mybits = 0;
    for (uint32_t k = 0; k < ns; ++k) {
        const uint32_t v = sym[k];
        if (v < 256u) { mybits += cl[v] >> 16; continue; }
        uint32_t eb, ev, eb2, ev2;
        const uint32_t lc = len_code(v - 253u, &eb, &ev), dc = dist_code((uint32_t)sym[++k] + 1u, &eb2, &ev2);
        mybits += (cl[lc] >> 16) + eb + (cd[dc] >> 16) + eb2;
    }
    uint32_t data_bits;
    const uint32_t hdr_bits = misc[kMiscHdrBits];
    const uint32_t my_off = hdr_bits + wg_scan<kPngThreads>(mybits, misc + kMiscScan, &data_bits);
    const uint32_t end_bits = hdr_bits + data_bits + (cl[256] >> 16);
    // non-final: an empty stored block (3 bits, pad, 00 00 FF FF) ends the segment on a byte boundary
    const uint32_t dyn_bytes = final ? (end_bits + 7u) / 8u : (end_bits + 3u + 7u) / 8u + 4u;
    const bool dyn = dyn_bytes < 5u + L;
    const uint32_t body = dyn ? dyn_bytes : 5u + L;
    if (dyn) {
        // the window becomes the bit buffer (the parse is over: every lane is past the scan's barriers)
        uint32_t *bb = reinterpret_cast<uint32_t *>(win);
        for (uint32_t i = tid; i < dyn_bytes / 4u + 2u; i += kPngThreads) bb[i] = 0u;
        __syncthreads();
        if (tid == 0u) {
            uint32_t pos = 0;
            put_bits(bb, pos, (final ? 1u : 0u) | (2u << 1), 3u); pos += 3u;
            put_bits(bb, pos, misc[kMiscHlit] - 257u, 5u); pos += 5u;
            put_bits(bb, pos, misc[kMiscHdist] - 1u, 5u); pos += 5u;
            const uint32_t hclen = misc[kMiscHclen];
            put_bits(bb, pos, hclen - 4u, 4u); pos += 4u;
            for (uint32_t k = 0; k < hclen; ++k) { put_bits(bb, pos, cc[kClOrder[k]] >> 16, 3u); pos += 3u; }
            const uint32_t *rle = head + kRle;
            for (uint32_t k = 0; k < misc[kMiscNrle]; ++k) {
                const uint32_t a = rle[k] & 255u, x = rle[k] >> 8, e = a == 16u ? 2u : a == 17u ? 3u : a == 18u ? 7u : 0u;
                put_bits(bb, pos, cc[a] & 0xffffu, cc[a] >> 16); pos += cc[a] >> 16;
                put_bits(bb, pos, x, e); pos += e;
            }
            put_bits(bb, hdr_bits + data_bits, cl[256] & 0xffffu, cl[256] >> 16); // end of block
            if (!final) {
                const uint32_t b = (end_bits + 3u + 7u) / 8u; // (the stored block's 3 header bits are zeros)
                atomicOr(&bb[(b + 2u) >> 2], 0xFFu << (8u * ((b + 2u) & 3u)));
                atomicOr(&bb[(b + 3u) >> 2], 0xFFu << (8u * ((b + 3u) & 3u)));
            }
        }
        uint32_t pos = my_off;
        for (uint32_t k = 0; k < ns; ++k) {
            const uint32_t v = sym[k];
            if (v < 256u) { put_bits(bb, pos, cl[v] & 0xffffu, cl[v] >> 16); pos += cl[v] >> 16; continue; }
            uint32_t eb, ev, eb2, ev2;
            const uint32_t lc = len_code(v - 253u, &eb, &ev), dc = dist_code((uint32_t)sym[++k] + 1u, &eb2, &ev2);
            put_bits(bb, pos, cl[lc] & 0xffffu, cl[lc] >> 16); pos += cl[lc] >> 16;
            put_bits(bb, pos, ev, eb); pos += eb;
            put_bits(bb, pos, cd[dc] & 0xffffu, cd[dc] >> 16); pos += cd[dc] >> 16;
            put_bits(bb, pos, ev2, eb2); pos += eb2;
        }
    }
    // ---- the chunk: length, "IDAT", [zlib header], body, CRC-32 of type + payload ----
    uint32_t *crc_tab = reinterpret_cast<uint32_t *>(png_lds + kLdsPrev);
    __syncthreads();
    crc_tab[tid] = kCrc.byte[tid];
    __syncthreads();
    const uint32_t zh = first ? 2u : 0u, plen = zh + body;
    const uint8_t flevel = jb.level >= 2u ? 3u : jb.level == 1u ? 2u : 0u;
    const uint32_t cmf_flg = (0x78u << 8) | (flevel << 6);
    const uint32_t zflg = (cmf_flg + (31u - cmf_flg % 31u) % 31u) & 255u;
    uint8_t *chunk = jb.chunks + (size_t)s * kPngSegOutBytes;
    const uint32_t per = (plen + kPngThreads - 1u) / kPngThreads, j0 = min(tid * per, plen), j1 = min(j0 + per, plen);
    uint32_t r = 0;
    for (uint32_t j = j0; j < j1; ++j) {
        uint32_t b;
        if (j < zh) b = j == 0u ? 0x78u : zflg;
        else {
            const uint32_t k = j - zh;
            if (dyn) b = win[k];
            else if (k >= 5u) b = win[H + k - 5u];
            else b = k == 0u ? (final ? 1u : 0u) : k == 1u ? (L & 255u) : k == 2u ? (L >> 8) : k == 3u ? (~L & 255u) : ((~L >> 8) & 255u);
        }
        chunk[8u + j] = (uint8_t)b;
        r = crc_tab[(r ^ b) & 255u] ^ (r >> 8);
    }
    if (j1 > j0) r = crc_mulmod(crc_shift_op(plen - j1), r);
    r = wave_xor(r);
    __syncthreads();
    if ((tid & 63u) == 0u) misc[kMiscScan + (tid >> 6)] = r;
    __syncthreads();
    if (tid == 0u) {
        uint32_t x = misc[kMiscScan] ^ misc[kMiscScan + 1] ^ misc[kMiscScan + 2] ^ misc[kMiscScan + 3];
        const uint8_t type[4] = {'I', 'D', 'A', 'T'};
        const uint32_t s0 = crc_bytes(0xffffffffu, type, 4u);
        const uint32_t crc = ~(crc_mulmod(crc_shift_op(plen), s0) ^ x);
        put_be32(chunk, plen);
        for (int k = 0; k < 4; ++k) chunk[4 + k] = type[k];
        put_be32(chunk + 8u + plen, crc);
        uint32_t *rec = jb.recs + (size_t)s * 4u;
        rec[0] = 12u + plen; rec[1] = (uint32_t)adler_a; rec[2] = (uint32_t)adler_b; rec[3] = L;
    }
}

// ---------------------------------------------------------------- kernel 3: the file --

__global__ __launch_bounds__(kPngThreads) void png_frame_kernel(const PngJob *__restrict__ jobs)
{
    __shared__ uint64_t s_red[kPngThreads / 64u];
    const PngJob &jb = jobs[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    uint64_t sz = 0, sa = 0, sb = 0;
    for (uint32_t s = tid; s < jb.nseg; s += kPngThreads) {
        const uint32_t *rec = jb.recs + (size_t)s * 4u;
        sz += rec[0];
        sa += rec[1];
        // segment at offset o of n bytes: its bytes count (n - o - L) times more in B than in its own partial sum
        const uint64_t after = jb.fbytes - (uint64_t)s * kPngSegBytes - rec[3];
        sb += (rec[2] + (after % 65521u) * rec[1]) % 65521u;
    }
    const uint64_t chunks = wg_sum64(sz, s_red);
    const uint64_t A = (1u + wg_sum64(sa, s_red)) % 65521u;
    const uint64_t B = (wg_sum64(sb, s_red) + jb.fbytes) % 65521u;
    const uint64_t total = 8u + 25u + chunks + 16u + 12u;
    if (total > jb.dst_cap) {
        if (tid == 0u) jb.result[1] = 0u;
        return;
    }
    uint8_t *d = jb.dst;
    if (tid == 0u) {
        const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
        for (int k = 0; k < 8; ++k) d[k] = sig[k];
        uint8_t ih[17] = {'I', 'H', 'D', 'R'};
        put_be32(ih + 4, jb.w); put_be32(ih + 8, jb.h);
        ih[12] = 8; ih[13] = jb.c == 1u ? 0 : jb.c == 2u ? 4 : jb.c == 3u ? 2 : 6; ih[14] = 0; ih[15] = 0; ih[16] = 0;
        put_be32(d + 8, 13u);
        for (int k = 0; k < 17; ++k) d[12 + k] = ih[k];
        put_be32(d + 29, ~crc_bytes(0xffffffffu, ih, 17u));
        uint8_t *t = d + 33u + chunks;
        uint8_t ad[8] = {'I', 'D', 'A', 'T'};
        put_be32(ad + 4, (uint32_t)((B << 16) | A));
        put_be32(t, 4u);
        for (int k = 0; k < 8; ++k) t[4 + k] = ad[k];
        put_be32(t + 12, ~crc_bytes(0xffffffffu, ad, 8u));
        const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int k = 0; k < 12; ++k) t[16 + k] = iend[k];
    }
    uint64_t off = 33u;
    for (uint32_t s = 0; s < jb.nseg; ++s) {
        const uint32_t n = jb.recs[(size_t)s * 4u];
        const uint8_t *src = jb.chunks + (size_t)s * kPngSegOutBytes;
        for (uint32_t i = tid; i < n; i += kPngThreads) d[off + i] = src[i];
        off += n;
    }
    if (tid == 0u) jb.result[1] = (uint32_t)total;
}

} // namespace

hipError_t launch_png_encode(const PngJob *jobs, uint32_t njobs, uint32_t total_rows, uint32_t total_segs, hipStream_t st)
{
    if (!njobs || !total_rows || !total_segs) return hipSuccess;
    static std::atomic<uint64_t> attr_set{0};
    if (hipError_t e = set_max_lds_once(attr_set, (int)kDeflateLds, {reinterpret_cast<const void *>(&png_deflate_kernel)}); e != hipSuccess) return e;
    const uint32_t rows_per_wg = kPngThreads / 64u;
    hipLaunchKernelGGL(png_filter_kernel, dim3((total_rows + rows_per_wg - 1u) / rows_per_wg), dim3(kPngThreads), 0, st, jobs, njobs, total_rows);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_deflate_kernel, dim3(total_segs), dim3(kPngThreads), kDeflateLds, st, jobs, njobs);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_frame_kernel, dim3(njobs), dim3(kPngThreads), 0, st, jobs);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace fl
