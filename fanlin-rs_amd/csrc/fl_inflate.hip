// fl_inflate.hip -- the deflate stream of a PNG source inflated on the device: one workgroup of kInfThreads threads per picture.
//
// Deflate blocks are taken in sequence (a block's header lies behind the previous block's end).  The header's words are loaded into
// LDS; BFINAL and BTYPE are the same for every thread; one lane reads a dynamic block's code lengths and builds the two tables
// (inf_dynamic_header), the fixed code's tables are built once.  A stored block is a cooperative copy.
//
// A block's tokens are decoded in strips of kInfSubs subsequences of kInfSubBits bits, the strip's words in an LDS window:
//   1. synchronisation: thread t walks subsequence t from a guessed start bit and stores where the first token behind it begins
//      (or: end-of-block met / invalid).  Then every thread whose predecessor's state changed walks again from that state, until no state
//      changes: after round r the first r states are exact, so a valid stream always settles, in at most kInfSubs rounds.
//   2. a workgroup scan of the bytes each subsequence's tokens write gives its output offset; a total beyond what IHDR implies is a "no"
//      before anything is written.
//   3. write and resolve: every thread goes on through its tokens, stores literals, and copies a match once its source lies below
//      `done`, the output position of the first match of the strip not copied yet (inf_ready).  A round ends with __threadfence() +
//      __syncthreads(), and what another wave wrote is read with device-scope loads (the hand-off png_unfilter_kernel uses); `done` is
//      the LDS minimum of the pending matches.  The first pending match is always ready, so every round copies at least one.  A chain of
//      matches that each need the one before (run-length style data) is copied one match per round: correct, and slow.
// Behind the final block: the length, the Adler-32 (summed by 16-byte pieces, inf_adler_piece) and every row's filter byte are checked.
// On any "no" the filter byte of every row is set to 0, so the unfilter kernel, which runs on the batch regardless, sees only 0..4.
//
// Nothing passes between workgroups.  Everything read from the stream is held against its bound before it indexes anything: window and
// payload reads (inf_peek clamps), table indices (inf_symbol), code-length counts (inf_build), output offsets (the scan, and `cap` in
// inf_resolve).  Every loop makes progress: a walk by at least a bit per token, a strip by kInfStripBits bits or to the end of its block, a
// block by at least its three header bits, a resolve round by at least one match.
#include "fl_inflate.h"

#include <stddef.h>

namespace fl {

namespace {

struct alignas(16) InfLds {
    uint32_t window[kInfWindowWords]; // the strip's words (a block header's words; at the end the Adler sums)
    uint32_t state[kInfSubs + 1];     // [t]: where subsequence t starts, [t + 1]: what its walk left
    InfTable fixed_lit, fixed_dist, lit, dist, cl;
    uint8_t lengths[320];
    uint32_t wsum[kInfThreads / 64u];
    uint32_t hdr_next;                // the bit behind a dynamic block's header, 0 = damaged
    uint32_t first;                   // the first subsequence that met the end of the block (or an invalid token)
    uint32_t done_next[3];            // the pending matches' minimum, one slot per round modulo 3
    uint32_t fail;
};
static_assert(sizeof(uint64_t) * 2u * kInfThreads <= sizeof(uint32_t) * kInfWindowWords, "the Adler sums fit the window");

// f(row's filter byte offset) for every row of the picture, or of its seven passes
template <typename F> __device__ __forceinline__ void for_each_row(const PngBlobHeader &H, uint32_t t, F f)
{
    const uint32_t bits = png_pixel_bits(H);
    for (uint32_t p = 0; p < (H.interlaced ? kAdam7Passes : 1u); ++p) {
        const Adam7Pass P = H.interlaced ? adam7_pass(H.width, H.height, bits, p) : Adam7Pass{H.width, H.height, H.row_bytes, 0, 0};
        if (!P.w || !P.h) continue;
        const uint64_t stride = 1u + (uint64_t)P.row_bytes;
        for (uint32_t y = t; y < P.h; y += kInfThreads) f(P.scan_off + (uint64_t)y * stride);
    }
}

// The whole stream; returns 0 or kInfErr*, the same value in every thread.
__device__ uint32_t inflate_picture(InfLds &s, const PngBlobHeader &H, const uint32_t *__restrict__ words, uint32_t payload, uint32_t expected, uint8_t *out)
{
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t nwords = ((uint64_t)payload + kPngzPad) / 4u, total_bits = (uint64_t)payload * 8u;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words);
    // zlib header (RFC 1950): deflate, window <= 32 KB, check bits, no preset dictionary
    if (payload < 2u) return kInfErrZlibHeader;
    {
        const uint32_t cmf = bytes[0], flg = bytes[1];
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return kInfErrZlibHeader;
    }
    if (t == 0) inf_fixed_tables(s.fixed_lit, s.fixed_dist, s.lengths);
    __syncthreads();
    uint64_t P = 16;
    uint32_t obase = 0;
    for (bool last = false; !last;) {
        if (total_bits - P < 3u) return kInfErrTruncated;
        const uint64_t hw = P >> 5;
        const uint32_t hb = (uint32_t)P & 31u;
        for (uint32_t k = t; k < kInfHeaderWords; k += kInfThreads) s.window[k] = hw + k < nwords ? words[hw + k] : 0u;
        __syncthreads();
        const uint64_t hv = inf_peek(s.window, kInfHeaderWords, hb);
        last = (hv & 1u) != 0;
        const uint32_t type = (uint32_t)(hv >> 1) & 3u;
        if (type == 3u) return kInfErrBlockType;
        if (type == 0u) {
            const uint64_t at = (P + 3u + 7u) >> 3;
            if (at + 4u > payload) return kInfErrTruncated;
            const uint32_t len = bytes[at] | (uint32_t)bytes[at + 1] << 8, nlen = bytes[at + 2] | (uint32_t)bytes[at + 3] << 8;
            if ((len ^ nlen) != 0xffffu) return kInfErrStored;
            if (len > payload - at - 4u) return kInfErrTruncated;
            if (len > expected - obase) return kInfErrTooLong;
            for (uint32_t i = t; i < len; i += kInfThreads) out[obase + i] = bytes[at + 4u + i];
            obase += len;
            P = (at + 4u + len) * 8u;
            __threadfence();
            __syncthreads();
            continue;
        }
        const InfTable *L = &s.fixed_lit, *D = &s.fixed_dist;
        if (type == 2u) {
            const uint64_t rem = total_bits - (hw << 5);
            if (t == 0) s.hdr_next = inf_dynamic_header(s.window, kInfHeaderWords, hb + 3u, rem > (1u << 28) ? 1u << 28 : (uint32_t)rem, s.cl, s.lit, s.dist, s.lengths);
            __syncthreads();
            const uint32_t q = s.hdr_next;
            if (!q) return kInfErrDynamicHeader;
            P = (hw << 5) + q;
            L = &s.lit; D = &s.dist;
        } else {
            P += 3u;
        }
        __syncthreads(); // the header's words have been read: the window is the strips' from here on
        for (bool in_block = true; in_block;) {
            const uint64_t wb = P >> 5;
            const uint32_t base = (uint32_t)P & 31u;
            for (uint32_t k = t; k < kInfWindowWords; k += kInfThreads) s.window[k] = wb + k < nwords ? words[wb + k] : 0u;
            const uint64_t rem = total_bits - (wb << 5);
            const uint32_t limit = rem > (1u << 28) ? 1u << 28 : (uint32_t)rem;
            const uint32_t bound = base + (t + 1u) * kInfSubBits;
            s.state[t] = base + t * kInfSubBits;
            if (t == 0) { s.first = kInfNever; s.done_next[0] = kInfNever; }
            __syncthreads();
            // ---- 1. synchronisation
            uint32_t seen = kInfNever, cnt = 0, ntok = 0;
            bool settled = false;
            for (uint32_t round = 0; round < kInfSubs + 2u; ++round) {
                const uint32_t in = s.state[t];
                __syncthreads();
                int changed = 0;
                if (in != seen) {
                    seen = in;
                    uint32_t st = kInfDead;
                    cnt = 0;
                    if (!(in & kInfFlags)) st = inf_walk(*L, *D, s.window, kInfWindowWords, in, bound, limit, cnt, ntok);
                    s.state[t + 1u] = st;
                    changed = 1;
                }
                if (!__syncthreads_or(changed)) { settled = true; break; }
            }
            if (!settled) return kInfErrRounds;
            // ---- 2. where the block ends, and every subsequence's output offset
            if (s.state[t + 1u] & (kInfEob | kInfInvalid)) atomicMin(&s.first, t);
            uint32_t inc = cnt;
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const uint32_t v = __shfl_up(inc, d, 64);
                if (lane >= d) inc += v;
            }
            if (lane == 63u) s.wsum[wave] = inc;
            __syncthreads();
            const uint32_t e = s.first;
            if (e != kInfNever && (s.state[e + 1u] & kInfInvalid)) return kInfErrCode;
            uint32_t woff = 0, total = 0;
            for (uint32_t w = 0; w < kInfThreads / 64u; ++w) { if (w < wave) woff += s.wsum[w]; total += s.wsum[w]; }
            if (total > expected - obase) return kInfErrTooLong;
            // ---- 3. write and resolve
            uint32_t p = seen, o = obase + woff + inc - cnt, done = obase;
            bool fin = (seen & kInfFlags) != 0;
            for (uint32_t rr = 0;; ++rr) {
                if (rr > kInfStripBits + 1u) return kInfErrRounds;
                if (t == 0) s.done_next[(rr + 1u) % 3u] = kInfNever;
                if (!fin) {
                    const int r = inf_resolve(*L, *D, s.window, kInfWindowWords, p, bound, o, done, out, expected);
                    // (no match is ever pending at output position 0 -- its distance would reach before the start -- so 0 in the round's
                    // slot says "failed": one word per round, read by every thread behind the same barrier)
                    if (r == kInfPending) atomicMin(&s.done_next[rr % 3u], o);
                    else { fin = true; if (r == kInfFail) atomicMin(&s.done_next[rr % 3u], 0u); }
                }
                __threadfence();
                __syncthreads();
                const uint32_t nx = s.done_next[rr % 3u];
                if (nx == 0u) return kInfErrDistance;
                if (nx == kInfNever) break;
                done = nx;
            }
            obase += total;
            if (e != kInfNever) { P = (wb << 5) + (s.state[e + 1u] & ~kInfFlags); in_block = false; }
            else P = (wb << 5) + s.state[kInfSubs];
            __syncthreads(); // states and window are rewritten by the next strip (or header)
        }
    }
    // ---- behind the final block: length, check value, filter bytes
    if (obase != expected) return kInfErrTooShort;
    const uint64_t at = (P + 7u) >> 3;
    if (at + 4u > payload) return kInfErrTruncated;
    const uint32_t want = (uint32_t)bytes[at] << 24 | (uint32_t)bytes[at + 1] << 16 | (uint32_t)bytes[at + 2] << 8 | bytes[at + 3];
    uint64_t s1 = 0, s2 = 0;
    for (uint32_t j = t * 16u; j < expected; j += kInfThreads * 16u) {
        const uint32_t k = expected - j < 16u ? expected - j : 16u;
        alignas(4) uint8_t d[16];
        if (k == 16u) {
            for (uint32_t q = 0; q < 4u; ++q) {
                const uint32_t v = __hip_atomic_load(reinterpret_cast<const uint32_t *>(out + j) + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                d[4u * q] = (uint8_t)v; d[4u * q + 1u] = (uint8_t)(v >> 8); d[4u * q + 2u] = (uint8_t)(v >> 16); d[4u * q + 3u] = (uint8_t)(v >> 24);
            }
        } else {
            for (uint32_t q = 0; q < k; ++q) d[q] = inf_load(out + j + q);
        }
        inf_adler_piece(s1, s2, d, k, (expected - j) % kAdlerMod);
    }
    uint64_t *sums = reinterpret_cast<uint64_t *>(s.window);
    sums[2u * t] = s1 % kAdlerMod; sums[2u * t + 1u] = s2 % kAdlerMod;
    if (t == 0) s.fail = 0;
    __syncthreads();
    if (t == 0) {
        uint64_t a = 0, b = 0;
        for (uint32_t k = 0; k < kInfThreads; ++k) { a += sums[2u * k]; b += sums[2u * k + 1u]; }
        if (inf_adler_finish(a, b, expected) != want) s.fail = kInfErrAdler;
    }
    bool bad = false;
    for_each_row(H, t, [&](uint64_t off) { bad |= off < expected && inf_load(out + off) > 4u; });
    __syncthreads();
    if (bad) atomicMax(&s.fail, (uint32_t)kInfErrFilterByte);
    __syncthreads();
    return s.fail;
}

__global__ __launch_bounds__(kInfThreads) void png_inflate_kernel(const InfJob *__restrict__ jobs)
{
    __shared__ InfLds s;
    const InfJob J = jobs[blockIdx.x];
    const uint32_t t = threadIdx.x;
    const PngBlobHeader &H = *reinterpret_cast<const PngBlobHeader *>(J.stage);
    // the header the unfilter / expand / Adam7 kernels read, as the host path would have written it
    {
        const uint32_t *from = reinterpret_cast<const uint32_t *>(J.stage);
        uint32_t *to = reinterpret_cast<uint32_t *>(J.scratch);
        for (uint32_t k = t; k < sizeof(PngBlobHeader) / 4u; k += kInfThreads) {
            uint32_t v = from[k];
            if (k == offsetof(PngBlobHeader, magic) / 4u) v = kPngMagic;
            if (k == offsetof(PngBlobHeader, total_bytes) / 4u) v = (uint32_t)sizeof(PngBlobHeader) + J.expected;
            to[k] = v;
        }
    }
    uint8_t *out = J.scratch + sizeof(PngBlobHeader);
    const uint32_t err = inflate_picture(s, H, reinterpret_cast<const uint32_t *>(J.stage + sizeof(PngBlobHeader)), J.payload_bytes, J.expected, out);
    if (err) for_each_row(H, t, [&](uint64_t off) { if (off < J.expected) out[off] = 0; });
    if (t == 0) *J.err = err;
}

} // namespace

hipError_t launch_png_inflate(const InfJob *jobs, uint32_t njobs, hipStream_t st)
{
    if (!njobs) return hipSuccess;
    hipLaunchKernelGGL(png_inflate_kernel, dim3(njobs), dim3(kInfThreads), 0, st, jobs);
    return hipGetLastError();
}

} // namespace fl
