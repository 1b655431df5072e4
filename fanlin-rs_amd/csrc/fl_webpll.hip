// fl_webpll.hip -- the lossless WebP encoder on gfx950, so that what leaves the GPU for `webp=true&quality=100` is the
// finished WebP file.
//
// Replaces `image`'s lossless WebP encoder (image-webp 0.2.1) for q == 100 (reference src/handler.rs:286-292, the picture
// converted by into_rgba8()).  The stream restates that encoder's layout: RIFF / VP8L, subtract-green,
// a predictor transform that is T (the pixel above) everywhere and L on row 0, one group of five prefix codes, no colour cache,
// and runs of the previous pixel (distance 1, at most 4096 long) as the only backward references.  Code lengths come from the
// length-limited builder the PNG deflate uses (fl_huff_build.h); the bytes are not pinned to the crate's, the pixels a decoder
// gets back are identical.  Integer only: the same bytes on every path and every run.
//
// Eight launches per batch; inside a launch no workgroup waits on another.  A picture's pixels are cut into tiles of
// kWebpllTile in raster order:
//   webpll_resid_kernel   per tile: residuals (RGBA, green subtracted, predicted) to scratch; the tile's last run start
//                         (a pixel that differs from its predecessor).
//   webpll_carry_kernel   per picture: the run start carried into every tile (exclusive prefix max); clears the histograms.
//   webpll_token_kernel   per tile: each pixel's distance k from its run start says what it is: a literal iff k mod 4097 == 0,
//                         the end of a backward reference of length k mod 4097 if that is 4096 or the run ends here, else
//                         inside one.  Histograms in LDS, added into the picture's.
//   webpll_code_kernel    per picture: one wave per code builds it (15 bits) and its code-length code (7 bits) and writes the
//                         code's header bits; one lane joins the header.
//   webpll_bits_kernel    per tile: the bits of its tokens.
//   webpll_scan_kernel    per picture: each tile's bit offset (exclusive scan after the header); the header and zeros into the
//                         bit stream.
//   webpll_place_kernel   per tile: every thread's tokens placed after a scan, ORed into an LDS copy of the tile's words; the
//                         words out (the two it may share with its neighbours by atomicOr).
//   webpll_frame_kernel   per picture: RIFF and chunk headers, the stream, the pad byte; the length (or 0 if the file does not
//                         fit dst_cap) into the result word.
// Every kernel is a template on the job mode (fl_webpll.h).  The alpha-plane instantiations code the alpha plane of a lossy WebP
// picture for its ALPH chunk (fl_vp8.hip): one byte per pixel read as ARGB (255, 0, a, 0), no VP8L header and no subtract-green in
// front of the predictor transform, no framing -- webpll_frame_kernel leaves the stream's byte count in front of the stream.  They
// return at once for a picture the planes launch found opaque.  The file-mode instantiations are the kernels as they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_huff_build.h"
#include "fl_types.h"
#include "fl_wave.h"
#include "fl_webpll.h"

namespace fl {

namespace {

constexpr uint32_t kPx = kWebpllTile / kWebpllThreads; // pixels per thread in the per-tile kernels (contiguous)
static_assert(kPx == 16u, "four 16-byte loads of residuals, two of tokens");
// the four alphabets side by side: green + lengths (280), red, blue, alpha (256 each)
constexpr uint32_t kOffG = 0, kOffR = 280, kOffB = 536, kOffA = 792, kAlph = 1048;
// per-picture scratch (WebpJob::pic): histograms | codes | header bits | [0] header bits, [2..3] total bits
constexpr uint32_t kPicHist = 0, kPicCodes = kAlph, kPicHdr = 2112, kPicHdrWords = 256, kPicMeta = kPicHdr + kPicHdrWords;
static_assert(kPicMeta + 4u <= kWebpllPicWords, "per-picture scratch");
constexpr uint32_t kTokLiteral = 0x8000u;
constexpr uint32_t kMaxRun = 4096u;
// a tile's bits (at most 60 per pixel) from any bit position of its first word
constexpr uint32_t kTileWords = (kWebpllTile * 60u + 31u + 31u) / 32u;

__constant__ uint32_t kAOff[4] = {kOffG, kOffR, kOffB, kOffA};
__constant__ uint32_t kASize[4] = {280u, 256u, 256u, 256u};
__constant__ uint8_t kClOrder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

// ---------------------------------------------------------------- helpers --

// exclusive scan (maximum) over the workgroup, the counterpart of fl_wave.h wg_scan; *all = the maximum of all
__device__ __forceinline__ uint32_t wg_excl_max(uint32_t v, uint32_t *s_w, uint32_t *all)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc = max(inc, t);
    }
    const uint32_t before = __shfl_up(inc, 1, 64);
    __syncthreads();
    if (lane == 63u) s_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0, m = 0;
#pragma unroll
    for (uint32_t i = 0; i < kWebpllThreads / 64u; ++i) { const uint32_t t = s_w[i]; if (i < wave) base = max(base, t); m = max(m, t); }
    *all = m;
    return max(base, lane ? before : 0u);
}

// LSB-first bits into 32-bit words from bit `pos` on; single writer per word except the first and the last (atomicOr)
struct BitSink {
    uint32_t *w;
    uint32_t wi, n;
    uint64_t acc;
    bool shared_ends;
    __device__ BitSink(uint32_t *words, uint32_t pos, bool ends) : w(words), wi(pos >> 5), n(pos & 31u), acc(0), shared_ends(ends) {}
    __device__ __forceinline__ void store(uint32_t v) { if (shared_ends) atomicOr(&w[wi], v); else w[wi] = v; ++wi; }
    __device__ __forceinline__ void put(uint32_t v, uint32_t k)
    {
        acc |= (uint64_t)v << n;
        n += k;
        while (n >= 32u) { store((uint32_t)acc); acc >>= 32; n -= 32u; }
    }
    __device__ __forceinline__ uint32_t flush() { const uint32_t bits = wi * 32u + n; if (n) store((uint32_t)acc); return bits; }
};

// a simple code of one symbol: 0 bits per use
__device__ __forceinline__ void put_simple(BitSink &o, uint32_t sym)
{
    o.put(1u, 1u); o.put(0u, 1u);
    if (sym < 2u) { o.put(0u, 1u); o.put(sym, 1u); } else { o.put(1u, 1u); o.put(sym, 8u); }
}

// VP8L prefix coding of a length v in 1..4096: symbol, extra bits, extra value
__device__ __forceinline__ uint32_t prefix_code(uint32_t v, uint32_t *eb, uint32_t *ev)
{
    const uint32_t x = v - 1u;
    if (x < 4u) { *eb = 0; *ev = 0; return x; }
    const uint32_t nb = 31u - (uint32_t)__clz(x);
    *eb = nb - 1u; *ev = x & ((1u << (nb - 1u)) - 1u);
    return 2u * nb + ((x >> (nb - 1u)) & 1u);
}

__device__ __forceinline__ uint32_t clen(const uint32_t *code, uint32_t s) { return code[s] >> 16; }

__device__ __forceinline__ uint32_t token_bits(uint32_t tk, uint32_t r, const uint32_t *code)
{
    if (tk == kTokLiteral)
        return clen(code, kOffG + ((r >> 8) & 255u)) + clen(code, kOffR + ((r >> 16) & 255u)) + clen(code, kOffB + (r & 255u)) +
               clen(code, kOffA + (r >> 24));
    if (!tk) return 0;
    uint32_t eb, ev;
    const uint32_t s = prefix_code(tk, &eb, &ev);
    return clen(code, kOffG + 256u + s) + eb;
}

__device__ __forceinline__ void load16(const WebpJob &jb, uint32_t p0, uint32_t (&r)[kPx], uint32_t (&tk)[kPx], bool toks)
{
    const uint4 *q = reinterpret_cast<const uint4 *>(jb.res + p0);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) { const uint4 v = q[k]; r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w; }
    if (!toks) return;
    const uint4 *qt = reinterpret_cast<const uint4 *>(jb.tok + p0);
#pragma unroll
    for (uint32_t k = 0; k < 2u; ++k) {
        const uint4 v = qt[k];
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) { tk[8 * k + 2 * j] = u[j] & 0xffffu; tk[8 * k + 2 * j + 1] = u[j] >> 16; }
    }
}

// ---------------------------------------------------------------- kernel 1: residuals --

// an alpha-mode job of an opaque picture: nothing to code (uniform over the workgroup; read before any barrier)
template <bool ALPHA> __device__ __forceinline__ bool idle(const WebpJob &jb) { return ALPHA && (jb.result[0] & 1u) == 0u; }

// into_rgba8, then subtract green: ARGB with r - g and b - g.  ALPHA: the plane's sample as green, nothing subtracted.
template <bool ALPHA> __device__ __forceinline__ uint32_t load_argb(const WebpJob &jb, uint32_t x, uint32_t y)
{
    if (ALPHA) return 0xff000000u | ((uint32_t)jb.src[(size_t)y * jb.w + x] << 8);
    const uint8_t *p = jb.src + ((size_t)y * jb.w + x) * jb.c;
    uint32_t r, g, b, a;
    if (jb.c <= 2u) { r = g = b = p[0]; a = jb.c == 2u ? p[1] : 255u; }
    else { r = p[0]; g = p[1]; b = p[2]; a = jb.c == 4u ? p[3] : 255u; }
    return (a << 24) | (((r - g) & 255u) << 16) | (g << 8) | ((b - g) & 255u);
}

// per-channel a - b mod 256 (libwebp's VP8LSubPixels)
__device__ __forceinline__ uint32_t sub_pixels(uint32_t a, uint32_t b)
{
    const uint32_t ag = 0x00ff00ffu + (a & 0xff00ff00u) - (b & 0xff00ff00u);
    const uint32_t rb = 0xff00ff00u + (a & 0x00ff00ffu) - (b & 0x00ff00ffu);
    return (ag & 0xff00ff00u) | (rb & 0x00ff00ffu);
}

// the predictor transform with mode T everywhere: black for the first pixel, L on row 0, T below
template <bool ALPHA> __device__ __forceinline__ uint32_t residual(const WebpJob &jb, uint32_t i)
{
    const uint32_t y = i / jb.w, x = i - y * jb.w;
    const uint32_t p = load_argb<ALPHA>(jb, x, y);
    if (y) return sub_pixels(p, load_argb<ALPHA>(jb, x, y - 1u));
    return sub_pixels(p, x ? load_argb<ALPHA>(jb, x - 1u, 0u) : 0xff000000u);
}

template <bool ALPHA> __global__ __launch_bounds__(kWebpllThreads) void webpll_resid_kernel(const WebpJob *__restrict__ jobs, uint32_t njobs)
{
    __shared__ uint32_t s_res[kWebpllTile + 1u]; // [k] = residual of pixel base + k - 1
    __shared__ uint32_t s_w[kWebpllThreads / 64u];
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const WebpJob &jb = jobs[find_first_le(jobs, njobs, t, &WebpJob::tile0)];
    if (idle<ALPHA>(jb)) return;
    const uint32_t lt = t - jb.tile0, npix = jb.w * jb.h, base = lt * kWebpllTile;
    for (uint32_t k = tid; k <= kWebpllTile; k += kWebpllThreads) {
        const uint32_t i = base + k - 1u;
        if (base + k >= 1u && i < npix) {
            const uint32_t r = residual<ALPHA>(jb, i);
            s_res[k] = r;
            if (k) jb.res[i] = r;
        }
    }
    __syncthreads();
    uint32_t mx = 0;
    for (uint32_t k = tid; k < kWebpllTile; k += kWebpllThreads) {
        const uint32_t i = base + k;
        if (i < npix && (i == 0u || s_res[k + 1u] != s_res[k])) mx = i + 1u;
    }
    mx = wave_max(mx);
    if ((tid & 63u) == 0u) s_w[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0u) jb.tiles[lt].last = max(max(s_w[0], s_w[1]), max(s_w[2], s_w[3]));
}

// ---------------------------------------------------------------- kernel 2: run starts carried across tiles --

template <bool ALPHA> __global__ __launch_bounds__(kWebpllThreads) void webpll_carry_kernel(const WebpJob *__restrict__ jobs)
{
    __shared__ uint32_t s_w[kWebpllThreads / 64u];
    const WebpJob &jb = jobs[blockIdx.x];
    if (idle<ALPHA>(jb)) return;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kAlph; i += kWebpllThreads) jb.pic[kPicHist + i] = 0u;
    uint32_t run = 0;
    for (uint32_t b0 = 0; b0 < jb.ntiles; b0 += kWebpllThreads) {
        const uint32_t t = b0 + tid;
        uint32_t all;
        const uint32_t ex = wg_excl_max(t < jb.ntiles ? jb.tiles[t].last : 0u, s_w, &all);
        if (t < jb.ntiles) jb.tiles[t].carry = max(run, ex);
        run = max(run, all);
    }
}

// ---------------------------------------------------------------- kernel 3: tokens and histograms --

template <bool ALPHA> __global__ __launch_bounds__(kWebpllThreads) void webpll_token_kernel(const WebpJob *__restrict__ jobs, uint32_t njobs)
{
    __shared__ uint32_t s_hist[kAlph];
    __shared__ uint32_t s_first[kWebpllThreads], s_last[kWebpllThreads];
    __shared__ uint32_t s_edge[2];
    __shared__ uint32_t s_w[kWebpllThreads / 64u];
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const WebpJob &jb = jobs[find_first_le(jobs, njobs, t, &WebpJob::tile0)];
    if (idle<ALPHA>(jb)) return;
    const uint32_t lt = t - jb.tile0, npix = jb.w * jb.h, base = lt * kWebpllTile;
    for (uint32_t i = tid; i < kAlph; i += kWebpllThreads) s_hist[i] = 0u;
    const uint32_t p0 = base + tid * kPx;
    const bool act = p0 < npix; // (the scratch is padded to 64 pixels: a thread's 16 are readable once its first is)
    uint32_t r[kPx], tk[kPx];
#pragma unroll
    for (uint32_t k = 0; k < kPx; ++k) r[k] = 0u;
    if (act) load16(jb, p0, r, tk, false);
    s_first[tid] = r[0]; s_last[tid] = r[kPx - 1u];
    if (tid == 0u) {
        s_edge[0] = base ? jb.res[base - 1u] : 0u;
        s_edge[1] = base + kWebpllTile < npix ? jb.res[base + kWebpllTile] : 0u;
    }
    __syncthreads();
    const uint32_t prevr = tid ? s_last[tid - 1u] : s_edge[0];
    const uint32_t nextr = tid + 1u < kWebpllThreads ? s_first[tid + 1u] : s_edge[1];
    uint32_t mx = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPx; ++k) {
        const uint32_t i = p0 + k;
        if (i < npix && (i == 0u || r[k] != (k ? r[k - 1u] : prevr))) mx = i + 1u;
    }
    uint32_t all;
    uint32_t cur = max(jb.tiles[lt].carry, wg_excl_max(mx, s_w, &all)); // run start + 1 of the pixel before this thread's
#pragma unroll
    for (uint32_t k = 0; k < kPx; ++k) {
        const uint32_t i = p0 + k;
        tk[k] = 0u;
        if (i >= npix) continue;
        if (i == 0u || r[k] != (k ? r[k - 1u] : prevr)) cur = i + 1u;
        const uint32_t m = (i + 1u - cur) % (kMaxRun + 1u);
        if (m == 0u) {
            tk[k] = kTokLiteral;
            atomicAdd(&s_hist[kOffG + ((r[k] >> 8) & 255u)], 1u);
            atomicAdd(&s_hist[kOffR + ((r[k] >> 16) & 255u)], 1u);
            atomicAdd(&s_hist[kOffB + (r[k] & 255u)], 1u);
            atomicAdd(&s_hist[kOffA + (r[k] >> 24)], 1u);
        } else {
            const bool run_ends = i + 1u >= npix || (k + 1u < kPx ? r[k + 1u] : nextr) != r[k];
            if (m == kMaxRun || run_ends) {
                uint32_t eb, ev;
                tk[k] = m;
                atomicAdd(&s_hist[kOffG + 256u + prefix_code(m, &eb, &ev)], 1u);
            }
        }
    }
    if (act) {
        uint4 *q = reinterpret_cast<uint4 *>(jb.tok + p0);
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k)
            q[k] = make_uint4(tk[8 * k] | (tk[8 * k + 1] << 16), tk[8 * k + 2] | (tk[8 * k + 3] << 16), tk[8 * k + 4] | (tk[8 * k + 5] << 16),
                              tk[8 * k + 6] | (tk[8 * k + 7] << 16));
    }
    __syncthreads();
    for (uint32_t i = tid; i < kAlph; i += kWebpllThreads)
        if (s_hist[i]) atomicAdd(&jb.pic[kPicHist + i], s_hist[i]);
}

// ---------------------------------------------------------------- kernel 4: codes and header --

template <bool ALPHA> __global__ __launch_bounds__(kWebpllThreads) void webpll_code_kernel(const WebpJob *__restrict__ jobs)
{
    __shared__ uint32_t s_hist[kAlph], s_key[kAlph], s_sym[kAlph], s_code[kAlph];
    __shared__ uint32_t s_num[4][64];
    __shared__ uint32_t s_cl[4][4 * 19]; // per code: code-length histogram | keys | symbols | codes
    __shared__ uint32_t s_sec[4][68];    // per code: its part of the header (at most 2023 bits)
    __shared__ uint32_t s_secbits[4];
    __shared__ uint32_t s_hdr[kPicHdrWords];
    const WebpJob &jb = jobs[blockIdx.x];
    if (idle<ALPHA>(jb)) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < kAlph; i += kWebpllThreads) { s_hist[i] = jb.pic[kPicHist + i]; s_code[i] = 0u; }
    __syncthreads();
    // rank the used symbols of each alphabet by (count, symbol)
    for (uint32_t i = tid; i < kAlph; i += kWebpllThreads) {
        const uint32_t a = i < kOffR ? 0u : 1u + (i - kOffR) / 256u, off = kAOff[a], n = kASize[a], s = i - off, f = s_hist[i];
        if (!f) continue;
        uint32_t rank = 0;
        for (uint32_t u = 0; u < n; ++u) { const uint32_t fu = s_hist[off + u]; rank += (fu && (fu < f || (fu == f && u < s))) ? 1u : 0u; }
        s_key[off + rank] = f;
        s_sym[off + rank] = s;
    }
    __syncthreads();
    if (lane == 0u) { // one wave per code
        const uint32_t a = wave, off = kAOff[a], n = kASize[a];
        uint32_t used = 0;
        for (uint32_t s = 0; s < n; ++s) used += s_hist[off + s] ? 1u : 0u;
        BitSink o(s_sec[a], 0u, false);
        if (used <= 1u) {
            put_simple(o, used ? s_sym[off] : 0u);
        } else {
            huff_build(s_key + off, s_sym + off, (int)used, 15u, n, s_code + off, s_num[a]);
            uint32_t *ch = s_cl[a], *ck = ch + 19, *cs = ck + 19, *cc = cs + 19;
            for (uint32_t k = 0; k < 19u; ++k) { ch[k] = 0u; cc[k] = 0u; }
            for (uint32_t s = 0; s < n; ++s) ch[s_code[off + s] >> 16]++;
            uint32_t cused = 0;
            for (uint32_t k = 0; k < 19u; ++k) {
                if (!ch[k]) continue;
                uint32_t rank = 0;
                for (uint32_t u = 0; u < 19u; ++u) rank += (ch[u] && (ch[u] < ch[k] || (ch[u] == ch[k] && u < k))) ? 1u : 0u;
                ck[rank] = ch[k]; cs[rank] = k; ++cused;
            }
            huff_build(ck, cs, (int)cused, 7u, 19u, cc, s_num[a]);
            o.put(0u, 1u);
            o.put(15u, 4u); // 19 code-length code lengths
            for (uint32_t k = 0; k < 19u; ++k) o.put(cc[kClOrder[k]] >> 16, 3u);
            if (n == 256u) { o.put(1u, 1u); o.put(3u, 3u); o.put(254u, 8u); } // max_symbol = 2 + 254
            else o.put(0u, 1u);
            if (cused >= 2u) // (one used code-length symbol: the decoder reads no bits for it)
                for (uint32_t s = 0; s < n; ++s) { const uint32_t l = s_code[off + s] >> 16; o.put(cc[l] & 0xffffu, cc[l] >> 16); }
        }
        s_secbits[a] = o.flush();
    }
    __syncthreads();
    if (tid == 0u) {
        BitSink o(s_hdr, 0u, false);
        if (!ALPHA) { // (an ALPH payload starts at the transform bits, and its red and blue stay zero without subtract-green)
            o.put(0x2fu, 8u);
            o.put(jb.w - 1u, 14u); o.put(jb.h - 1u, 14u);
            o.put(1u, 1u);  // alpha is used (the encoder is handed Rgba8)
            o.put(0u, 3u);  // version
            o.put(5u, 3u);  // transform: subtract green
        }
        o.put(57u, 6u); // transform: predictor, 2^9 blocks
        o.put(0u, 1u);  // its sub-image: no colour cache, five one-symbol codes (mode 2 = T), 0 bits per block
        put_simple(o, 2u);
        for (int k = 0; k < 4; ++k) put_simple(o, 0u);
        o.put(0u, 3u);  // no more transforms, no colour cache, no meta prefix codes
        for (uint32_t a = 0; a < 4u; ++a) {
            const uint32_t nb = s_secbits[a];
            for (uint32_t k = 0; k < nb / 32u; ++k) o.put(s_sec[a][k], 32u);
            if (nb & 31u) o.put(s_sec[a][nb / 32u] & ((1u << (nb & 31u)) - 1u), nb & 31u);
        }
        put_simple(o, 1u); // distance: plane code 2, the left pixel
        jb.pic[kPicMeta] = o.flush();
    }
    __syncthreads();
    for (uint32_t i = tid; i < kAlph; i += kWebpllThreads) jb.pic[kPicCodes + i] = s_code[i];
    const uint32_t hw = (jb.pic[kPicMeta] + 31u) / 32u;
    for (uint32_t i = tid; i < hw; i += kWebpllThreads) jb.pic[kPicHdr + i] = s_hdr[i];
}

// ---------------------------------------------------------------- kernel 5: bits per tile --

template <bool ALPHA> __global__ __launch_bounds__(kWebpllThreads) void webpll_bits_kernel(const WebpJob *__restrict__ jobs, uint32_t njobs)
{
    __shared__ uint32_t s_code[kAlph];
    __shared__ uint32_t s_w[kWebpllThreads / 64u];
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const WebpJob &jb = jobs[find_first_le(jobs, njobs, t, &WebpJob::tile0)];
    if (idle<ALPHA>(jb)) return;
    const uint32_t lt = t - jb.tile0, npix = jb.w * jb.h, base = lt * kWebpllTile;
    for (uint32_t i = tid; i < kAlph; i += kWebpllThreads) s_code[i] = jb.pic[kPicCodes + i];
    __syncthreads();
    const uint32_t p0 = base + tid * kPx;
    uint32_t bits = 0;
    if (p0 < npix) {
        uint32_t r[kPx], tk[kPx];
        load16(jb, p0, r, tk, true);
#pragma unroll
        for (uint32_t k = 0; k < kPx; ++k)
            if (p0 + k < npix) bits += token_bits(tk[k], r[k], s_code);
    }
    uint32_t total;
    (void)wg_scan<kWebpllThreads>(bits, s_w, &total);
    if (tid == 0u) jb.tiles[lt].bits = total;
}

// ---------------------------------------------------------------- kernel 6: tile offsets, header into the stream --

template <bool ALPHA> __global__ __launch_bounds__(kWebpllThreads) void webpll_scan_kernel(const WebpJob *__restrict__ jobs)
{
    __shared__ uint32_t s_w[kWebpllThreads / 64u];
    const WebpJob &jb = jobs[blockIdx.x];
    if (idle<ALPHA>(jb)) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t hb = jb.pic[kPicMeta];
    uint64_t run = hb;
    for (uint32_t b0 = 0; b0 < jb.ntiles; b0 += kWebpllThreads) {
        const uint32_t t = b0 + tid;
        uint32_t total;
        const uint32_t ex = wg_scan<kWebpllThreads>(t < jb.ntiles ? jb.tiles[t].bits : 0u, s_w, &total);
        if (t < jb.ntiles) jb.tiles[t].off = run + ex;
        run += total;
    }
    if (tid == 0u) { jb.pic[kPicMeta + 2] = (uint32_t)run; jb.pic[kPicMeta + 3] = (uint32_t)(run >> 32); }
    const uint64_t words = min<uint64_t>((run + 31u) / 32u, jb.stream_words), hw = (hb + 31u) / 32u;
    for (uint64_t k = tid; k < words; k += kWebpllThreads) jb.stream[k] = k < hw ? jb.pic[kPicHdr + k] : 0u;
}

// ---------------------------------------------------------------- kernel 7: bits placed --

template <bool ALPHA> __global__ __launch_bounds__(kWebpllThreads) void webpll_place_kernel(const WebpJob *__restrict__ jobs, uint32_t njobs)
{
    __shared__ uint32_t s_code[kAlph];
    __shared__ uint32_t s_buf[kTileWords];
    __shared__ uint32_t s_w[kWebpllThreads / 64u];
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const WebpJob &jb = jobs[find_first_le(jobs, njobs, t, &WebpJob::tile0)];
    if (idle<ALPHA>(jb)) return;
    const uint32_t lt = t - jb.tile0, npix = jb.w * jb.h, base = lt * kWebpllTile;
    const uint64_t off = jb.tiles[lt].off;
    const uint32_t tbits = jb.tiles[lt].bits;
    if (!tbits) return;
    const uint32_t nwords = ((uint32_t)(off & 31u) + tbits + 31u) / 32u;
    for (uint32_t i = tid; i < kAlph; i += kWebpllThreads) s_code[i] = jb.pic[kPicCodes + i];
    for (uint32_t i = tid; i < nwords; i += kWebpllThreads) s_buf[i] = 0u;
    __syncthreads();
    const uint32_t p0 = base + tid * kPx;
    const bool act = p0 < npix;
    uint32_t r[kPx], tk[kPx];
    uint32_t bits = 0;
    if (act) {
        load16(jb, p0, r, tk, true);
#pragma unroll
        for (uint32_t k = 0; k < kPx; ++k) {
            if (p0 + k >= npix) tk[k] = 0u;
            bits += token_bits(tk[k], r[k], s_code);
        }
    }
    uint32_t total;
    const uint32_t my = wg_scan<kWebpllThreads>(bits, s_w, &total);
    if (act && bits) {
        BitSink o(s_buf, (uint32_t)(off & 31u) + my, true);
#pragma unroll
        for (uint32_t k = 0; k < kPx; ++k) {
            const uint32_t v = tk[k], x = r[k];
            if (v == kTokLiteral) {
                const uint32_t cg = s_code[kOffG + ((x >> 8) & 255u)], cr = s_code[kOffR + ((x >> 16) & 255u)];
                const uint32_t cb = s_code[kOffB + (x & 255u)], ca = s_code[kOffA + (x >> 24)];
                o.put(cg & 0xffffu, cg >> 16); o.put(cr & 0xffffu, cr >> 16); o.put(cb & 0xffffu, cb >> 16); o.put(ca & 0xffffu, ca >> 16);
            } else if (v) {
                uint32_t eb, ev;
                const uint32_t c = s_code[kOffG + 256u + prefix_code(v, &eb, &ev)];
                o.put(c & 0xffffu, c >> 16);
                o.put(ev, eb);
            }
        }
        (void)o.flush();
    }
    __syncthreads();
    // the first and the last word may hold a neighbour's bits (zeroed by webpll_scan_kernel); the others are this tile's alone
    const uint64_t w0 = off >> 5;
    for (uint32_t k = tid; k < nwords; k += kWebpllThreads) {
        const uint64_t g = w0 + k;
        if (g >= jb.stream_words) break;
        if (k == 0u || k + 1u == nwords) atomicOr(&jb.stream[g], s_buf[k]);
        else jb.stream[g] = s_buf[k];
    }
}

// ---------------------------------------------------------------- kernel 8: the file --

template <bool ALPHA> __global__ __launch_bounds__(kWebpllThreads) void webpll_frame_kernel(const WebpJob *__restrict__ jobs)
{
    const WebpJob &jb = jobs[blockIdx.x];
    if (idle<ALPHA>(jb)) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t bits = (uint64_t)jb.pic[kPicMeta + 2] | ((uint64_t)jb.pic[kPicMeta + 3] << 32);
    const uint64_t n = (bits + 7u) / 8u, file = 20u + n + (n & 1u);
    if (ALPHA) { // the stream stays where it is (its last byte's spare bits are zero); its length in front of it
        if (tid == 0u) *reinterpret_cast<uint32_t *>(jb.dst) = n > 4ull * jb.stream_words ? 0u : (uint32_t)n;
        return;
    }
    if (file > jb.dst_cap || n > 4ull * jb.stream_words) {
        if (tid == 0u) jb.result[1] = 0u;
        return;
    }
    uint8_t *d = jb.dst;
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(jb.stream);
    if (((uintptr_t)d & 3u) == 0u) {
        uint32_t *dw = reinterpret_cast<uint32_t *>(d + 20);
        for (uint64_t k = tid; k < n / 4u; k += kWebpllThreads) dw[k] = jb.stream[k];
        for (uint64_t k = (n & ~3ull) + tid; k < n; k += kWebpllThreads) d[20u + k] = sb[k];
    } else {
        for (uint64_t k = tid; k < n; k += kWebpllThreads) d[20u + k] = sb[k];
    }
    if (tid == 0u) {
        const uint32_t riff = (uint32_t)(file - 8u), len = (uint32_t)n;
        const uint8_t h[20] = {'R', 'I', 'F', 'F', (uint8_t)riff, (uint8_t)(riff >> 8), (uint8_t)(riff >> 16), (uint8_t)(riff >> 24),
                               'W', 'E', 'B', 'P', 'V', 'P', '8', 'L', (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)(len >> 16), (uint8_t)(len >> 24)};
        for (int k = 0; k < 20; ++k) d[k] = h[k];
        if (n & 1u) d[20u + n] = 0u;
        jb.result[1] = (uint32_t)file;
    }
}

} // namespace

template <bool ALPHA> static hipError_t launch_mode(const WebpJob *jobs, uint32_t njobs, uint32_t total_tiles, hipStream_t st)
{
    const dim3 blk(kWebpllThreads);
    hipLaunchKernelGGL(webpll_resid_kernel<ALPHA>, dim3(total_tiles), blk, 0, st, jobs, njobs);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(webpll_carry_kernel<ALPHA>, dim3(njobs), blk, 0, st, jobs);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(webpll_token_kernel<ALPHA>, dim3(total_tiles), blk, 0, st, jobs, njobs);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(webpll_code_kernel<ALPHA>, dim3(njobs), blk, 0, st, jobs);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(webpll_bits_kernel<ALPHA>, dim3(total_tiles), blk, 0, st, jobs, njobs);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(webpll_scan_kernel<ALPHA>, dim3(njobs), blk, 0, st, jobs);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(webpll_place_kernel<ALPHA>, dim3(total_tiles), blk, 0, st, jobs, njobs);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(webpll_frame_kernel<ALPHA>, dim3(njobs), blk, 0, st, jobs);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_webpll_encode(const WebpJob *jobs, uint32_t njobs, uint32_t total_tiles, hipStream_t st, uint32_t mode)
{
    if (!njobs || !total_tiles) return hipSuccess;
    return mode == kWebpllModeAlpha ? launch_mode<true>(jobs, njobs, total_tiles, st) : launch_mode<false>(jobs, njobs, total_tiles, st);
}

} // namespace fl
