// fl_webpdec.hip -- device half of the lossless WebP decode front end: the VP8L transforms inverted on the residual picture.
//
// The predictor transform is px(x, y) = res(x, y) + pred(L, T, TR, TL) per channel mod 256, with the mode taken from a
// sub-resolution image.  It is serial along a row (L) and down the picture (T, TL, TR); what is parallel is the anti-diagonal,
// and because of the top-RIGHT neighbour a row runs TWO pixels behind the row above it.
//
// webp_predict_kernel: one workgroup per picture, kWdWaves waves, the scheme of png_unfilter_kernel.  A wave owns a band of 64
// rows: lane r reconstructs pixel t - 2 r of row r at step t, keeps its own previous pixel (L) in a register and takes TR from
// lane r - 1 (__shfl_up of that lane's latest result); T and TL are what it took one and two steps earlier.  TR of a row's
// last pixel is pixel 0 of the lane's OWN row (the next dword in memory, as libwebp reads it).  All 14 predictions are
// computed on packed dwords and one is selected: no divergent branch in the step.  A band is walked in chunks of kWdChunk
// steps: the wave stages its slice of the chunk -- for row r the residuals of pixels [64 j - 2 r, 64 j - 2 r + 64) -- into LDS
// with coalesced dword loads, one row per lane, reconstructs in place, and writes the slice back with coalesced dword stores.
// The last row of a band is the row above the next band's lane 0: that wave reads it back from the output, pixels
// [64 j + 1, 64 j + 65) in chunk j, kWdLag = 3 chunk steps behind.  Band b runs on wave b % 8; with more than 8 bands wave 0
// continues with band 8 once it is free and band 7 is three chunks ahead, and so on.  Every wave runs the same number of chunk
// steps with one __syncthreads() each (idle steps included): no spin waits, no flags, nothing between workgroups.
//
// webp_run_kernel: the pointwise transforms (cross-colour, add-green, colour indexing), any run of them fused per output
// pixel, and the final dword -> R, G, B(, A) bytes conversion fused into the last run.
#include "fl_webpdec.h"

#include <algorithm>
#include <atomic>

#include "fl_types.h"

namespace fl {

namespace {

// stores of another wave of this workgroup, made visible by __threadfence() + __syncthreads(): read past the vector L1
__device__ __forceinline__ uint32_t load_coherent(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LDS traffic inside one wave (staging by all lanes, then each lane on its own row): instructions of a wave execute in
// order, the compiler must keep them so
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// four channels in a dword, a << 24 | r << 16 | g << 8 | b
__device__ __forceinline__ uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
__device__ __forceinline__ uint32_t add_px(uint32_t a, uint32_t b)
{
    return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}
__device__ __forceinline__ int32_t chan(uint32_t v, uint32_t k) { return (int32_t)((v >> (8u * k)) & 255u); }
__device__ __forceinline__ uint32_t clip255(int32_t v) { return (uint32_t)min(max(v, 0), 255); }

// the prediction of `mode` (0..15; 14 and 15 as 0, as libwebp decodes them)
__device__ __forceinline__ uint32_t predict(uint32_t mode, uint32_t L, uint32_t T, uint32_t TR, uint32_t TL)
{
    const uint32_t a_lt = avg2(L, T), a_ltl = avg2(L, TL), a_ttr = avg2(T, TR);
    // 11, Select: L if the sum over the channels of |T - TL| is below that of |L - TL|, else T
    const uint32_t sel = __builtin_amdgcn_sad_u8(T, TL, 0u) < __builtin_amdgcn_sad_u8(L, TL, 0u) ? L : T;
    uint32_t full = 0, half = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const int32_t l = chan(L, k), t = chan(T, k), tl = chan(TL, k), a = chan(a_lt, k);
        full |= clip255(l + t - tl) << (8u * k);           // 12
        half |= clip255(a + (a - tl) / 2) << (8u * k);     // 13: C division, towards zero
    }
    uint32_t p = 0xff000000u;                               // 0 (and 14, 15)
    p = mode == 1u ? L : p;
    p = mode == 2u ? T : p;
    p = mode == 3u ? TR : p;
    p = mode == 4u ? TL : p;
    p = mode == 5u ? avg2(avg2(L, TR), T) : p;
    p = mode == 6u ? a_ltl : p;
    p = mode == 7u ? a_lt : p;
    p = mode == 8u ? avg2(TL, T) : p;
    p = mode == 9u ? a_ttr : p;
    p = mode == 10u ? avg2(a_ltl, a_ttr) : p;
    p = mode == 11u ? sel : p;
    p = mode == 12u ? full : p;
    p = mode == 13u ? half : p;
    return p;
}

__global__ __launch_bounds__(kWdThreads) void webp_predict_kernel(const WebpPredictJob *__restrict__ jobs)
{
    extern __shared__ __align__(16) uint32_t s_wd[];
    const WebpPredictJob &J = jobs[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t w = J.width, h = J.height, bits = J.bits;
    const uint32_t mw = (w + (1u << bits) - 1u) >> bits;
    const uint32_t *__restrict__ res = J.res;
    const uint32_t *__restrict__ modes = J.modes;
    uint32_t *out = J.out;
    const uint32_t nc = (w + kWdSkew + kWdChunk - 1u) / kWdChunk;      // chunk steps per band: lane 63 reaches pixel w - 1 at step w - 1 + kWdSkew
    const uint32_t round = max(nc, kWdLag * kWdWaves);                 // chunk steps between a wave's consecutive bands
    const uint32_t nbands = (h + kWdBandRows - 1u) / kWdBandRows;
    const uint32_t last = nbands - 1u;
    const uint32_t trips = (last / kWdWaves) * round + kWdLag * (last % kWdWaves) + nc; // the last band's last chunk step: the same count for every wave
    uint32_t *wbase = s_wd + (size_t)wave * kWdBandRows * kWdPitch;
    uint32_t *mine = wbase + (size_t)lane * kWdPitch;
    uint32_t cur = 0, tr = 0, tp = 0, tl = 0, first = 0;
    const uint32_t *mrow = modes;
    constexpr uint32_t UN = 8u; // rows whose loads are in flight together

    for (uint32_t s = 0; s < trips; ++s) {
        // which band and chunk this wave is at (wave-uniform)
        const bool started = s >= kWdLag * wave;
        const uint32_t local = started ? s - kWdLag * wave : 0u;
        const uint32_t j = local % round, band = (local / round) * kWdWaves + wave;
        if (started && j < nc && band < nbands) {
            const uint32_t row0 = band * kWdBandRows, row = row0 + lane;
            const uint32_t nrows = min(kWdBandRows, h - row0);
            const bool row_ok = row < h;
            if (j == 0u) {
                cur = tp = tl = first = 0u;
                // lane 0's T at step 0 is pixel 0 of the row above the band: it enters as "TR of the step before"
                tr = (lane == 0u && row0 > 0u) ? load_coherent(out + (size_t)(row0 - 1u) * w) : 0u;
                mrow = modes + (size_t)((row_ok ? row : 0u) >> bits) * mw;
            }
            // ---- stage this chunk's slice of every row: row r holds the residuals of pixels [64 j - 2 r, 64 j - 2 r + 64), a dword
            // per lane; eight rows' loads are issued before the first LDS store, so their latencies overlap
            const int64_t x0 = (int64_t)kWdChunk * j + lane;
            for (uint32_t r0 = 0; r0 < nrows; r0 += UN) {
                uint32_t v[UN];
#pragma unroll
                for (uint32_t k = 0; k < UN; ++k) {
                    const uint32_t r = r0 + k;
                    const int64_t x = x0 - 2 * (int64_t)r;
                    v[k] = (r < nrows && x >= 0 && x < (int64_t)w) ? res[(size_t)(row0 + r) * w + (size_t)x] : 0u;
                }
#pragma unroll
                for (uint32_t k = 0; k < UN; ++k) {
                    const uint32_t r = r0 + k;
                    if (r < nrows) wbase[r * kWdPitch + lane] = v[k];
                }
            }
            // ---- the row above lane 0: pixels [64 j + 1, 64 j + 65) of the previous band's last row, one per lane -- lane 0's TR
            uint32_t above = 0;
            if (row0 > 0u) {
                const int64_t x = x0 + 1;
                if (x < (int64_t)w) above = load_coherent(out + (size_t)(row0 - 1u) * w + (size_t)x);
            }
            wave_lds_sync();
            // ---- kWdChunk steps of the anti-diagonal
#pragma unroll 4
            for (uint32_t i = 0; i < kWdChunk; ++i) {
                const uint32_t from_above = __shfl_up(cur, 1, 64), top = __shfl(above, (int)i, 64);
                tl = tp;
                tp = tr;
                tr = lane == 0u ? top : from_above;
                const int64_t x = (int64_t)kWdChunk * j + i - 2 * (int64_t)lane;
                const uint32_t xc = (uint32_t)min(max(x, (int64_t)0), (int64_t)w - 1);
                uint32_t mode = (mrow[xc >> bits] >> 8) & 15u;
                // edges: (0, 0) is mode 0, the rest of row 0 L, column 0 T
                mode = row == 0u ? (xc == 0u ? 0u : 1u) : (xc == 0u ? 2u : mode);
                if (row_ok && x >= 0 && x < (int64_t)w) {
                    const uint32_t right = xc == w - 1u ? first : tr; // past the row above's end: this row's pixel 0
                    cur = add_px(mine[i], predict(mode, cur, tp, right, tl));
                    mine[i] = cur;
                    first = xc == 0u ? cur : first;
                }
            }
            wave_lds_sync();
            // ---- write the slices back, a dword per lane
            for (uint32_t r = 0; r < nrows; ++r) {
                const int64_t x = x0 - 2 * (int64_t)r;
                if (x >= 0 && x < (int64_t)w) out[(size_t)(row0 + r) * w + (size_t)x] = wbase[r * kWdPitch + lane];
            }
        }
        __threadfence();   // the band's last row is read by another wave, from memory
        __syncthreads();
    }
}

__device__ __forceinline__ int32_t cc_delta(uint32_t t, uint32_t c) { return ((int32_t)(int8_t)t * (int32_t)(int8_t)c) >> 5; }

// One thread per output pixel of a run of pointwise inverse transforms.
__global__ __launch_bounds__(256) void webp_run_kernel(const WebpRunJob *__restrict__ jobs)
{
    const WebpRunJob &J = jobs[blockIdx.y];
    const uint32_t dw = J.dst_w, sw = J.src_w, shift = J.shift, nops = J.nops, oc = J.out_c;
    const uint32_t npx = dw * J.height; // below 2^29 (webp_parse_info)
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < npx; p += gridDim.x * 256u) {
        const uint32_t y = p / dw, x = p - y * dw;
        uint32_t cx = x >> shift; // the column at the packed width, until the colour indexing widens the picture
        uint32_t v = J.src[(size_t)y * sw + cx];
        for (uint32_t k = 0; k < nops; ++k) {
            const WebpOp &op = J.ops[k];
            if (op.type == kWtSubtractGreen) {
                const uint32_t g = (v >> 8) & 255u;
                v = (v & 0xff00ff00u) | (((v & 0x00ff00ffu) + (g << 16 | g)) & 0x00ff00ffu);
            } else if (op.type == kWtCrossColor) {
                const uint32_t bw = (op.width + (1u << op.bits) - 1u) >> op.bits;
                const uint32_t e = op.data[(size_t)(y >> op.bits) * bw + (cx >> op.bits)]; // r2b << 16 | g2b << 8 | g2r
                const uint32_t g = (v >> 8) & 255u;
                const uint32_t r = ((v >> 16) + (uint32_t)cc_delta(e, g)) & 255u;
                const uint32_t b = (v + (uint32_t)cc_delta(e >> 8, g) + (uint32_t)cc_delta(e >> 16, r)) & 255u; // with the NEW red
                v = (v & 0xff00ff00u) | r << 16 | b;
            } else { // colour indexing: 1 << shift pixels in the green byte, lowest bits first
                const uint32_t bpp = 8u >> shift;
                const uint32_t idx = (((v >> 8) & 255u) >> ((x & ((1u << shift) - 1u)) * bpp)) & ((1u << bpp) - 1u);
                v = op.data[idx]; // 256 entries: any index stays inside
                cx = x;
            }
        }
        if (oc == 0u) static_cast<uint32_t *>(J.dst)[p] = v;
        else {
            uint8_t *o = static_cast<uint8_t *>(J.dst) + (size_t)p * oc;
            if (oc == 4u) *reinterpret_cast<uint32_t *>(o) = ((v >> 16) & 255u) | (v & 0xff00u) | (v & 255u) << 16 | (v & 0xff000000u);
            else { o[0] = (uint8_t)(v >> 16); o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)v; }
        }
    }
}

} // namespace

hipError_t launch_webp_predict(const WebpPredictJob *jobs, uint32_t njobs, hipStream_t st)
{
    static std::atomic<uint64_t> lds_set{0};
    if (!njobs) return hipSuccess;
    const hipError_t e = set_max_lds_once(lds_set, (int)kWdLdsBytes, {(const void *)webp_predict_kernel});
    if (e != hipSuccess) return e;
    webp_predict_kernel<<<dim3(njobs), dim3(kWdThreads), kWdLdsBytes, st>>>(jobs);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_webp_run(const WebpRunJob *jobs, uint32_t njobs, uint32_t max_pixels, hipStream_t st)
{
    const uint32_t gx = std::min<uint32_t>(std::max<uint32_t>((max_pixels + 255u) / 256u, 1u), 4096u);
    for (uint32_t base = 0; base < njobs; base += 32768u) { // grid.y limit
        const uint32_t cnt = std::min<uint32_t>(32768u, njobs - base);
        webp_run_kernel<<<dim3(gx, cnt), dim3(256), 0, st>>>(jobs + base);
        FL_LAUNCH_CHECK();
    }
    return hipSuccess;
}

} // namespace fl
