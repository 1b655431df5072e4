// fl_vp8dec.hip -- the lossy WebP decoder behind the boolean coder on gfx950 (reference src/handler.rs:205-220: image-webp
// decodes the `VP8 ` chunk on the host).  fl_vp8dec_core.h holds all of the arithmetic, shared with the host twin
// (tests/vp8_src_host.cpp); this file is the choreography:
//   vp8dec_recon_kernel   one workgroup per picture, anti-diagonals d = x + 2 y one after the other, a wave per macroblock of the
//                         diagonal.  Per macroblock: Y2 block and DC predictions (4 lanes), 24 residual blocks (24 lanes), then the
//                         samples: chroma and one-mode luma in one sub-step over all lanes, a B_PRED macroblock's sixteen
//                         sub-blocks in sixteen (16 lanes each; the residuals are ready before the chain starts).
//   vp8dec_filter_kernel  the same schedule, two macroblocks a wave, eight steps a macroblock (left edge, inner vertical edges,
//                         top edge, inner horizontal edges), 32 lines a step.  Equal to raster order: the macroblocks of one
//                         diagonal touch disjoint samples, and everything a macroblock reads was finished on an earlier one.
//   vp8dec_alpha_kernel   one workgroup per picture: the ALPH filter undone (copy; row prefix sums; column sums; the gradient
//                         predictor as a wavefront, row r one sample behind row r - 1).
//   vp8dec_rgb_kernel     a thread per run of four pixels: fancy up-sampling and the 14-bit YUV -> RGB, interleaved bytes out.
// Every barrier sits in control flow that is uniform over the workgroup (the loop bounds come from the picture's size alone), and
// no wave waits on memory another one writes: a damaged blob yields wrong pixels, never a wait.  No use of the device error word.
// A lone large picture is latency-bound: one workgroup walks mbw + 2 mbh diagonals.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_vp8dec.h"
#include "fl_vp8dec_core.h"
#include "fl_wave.h"

namespace fl {
namespace {

// the macroblock rows that have a macroblock on diagonal d: y in [lo, lo + count), x = d - 2 y
__device__ __forceinline__ uint32_t diagonal(const Vp8DecPic &p, uint32_t d, uint32_t &lo)
{
    lo = d >= p.mbw ? (d - p.mbw + 2u) >> 1 : 0u;
    const uint32_t hi = min(p.mbh - 1u, d >> 1);
    return hi >= lo ? hi - lo + 1u : 0u;
}

__global__ __launch_bounds__(kVp8dThreads) void vp8dec_recon_kernel(const Vp8DecJob *__restrict__ jobs)
{
    __shared__ Vp8DecWork s_work[kVp8dWaves];
    const Vp8DecJob &jb = jobs[blockIdx.x];
    Vp8DecPic p;
    vp8d_pic(p, jb.blob, jb.planes);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    Vp8DecWork &w = s_work[wave];
    const uint32_t ndiag = p.mbw + 2u * (p.mbh - 1u);
    for (uint32_t d = 0; d < ndiag; ++d) {
        uint32_t lo;
        const uint32_t count = diagonal(p, d, lo);
        for (uint32_t base = 0; base < count; base += kVp8dWaves) {
            const bool active = base + wave < count;
            const uint32_t mby = active ? lo + base + wave : 0u, mbx = active ? d - 2u * mby : 0u;
            const Vp8MbRecord &r = p.recs[(uint64_t)mby * p.mbw + mbx];
            if (active && lane < 4u) vp8d_prepare(p, r, w, mbx, mby, lane);
            // one sub-step is enough unless a macroblock of this round has sub-block modes
            const uint32_t steps = __syncthreads_or(active && r.ymode == kVp8BPred) ? kVp8dSubSteps : 1u;
            if (active && lane < 24u) vp8d_residual(p, r, w, lane);
            __syncthreads();
            for (uint32_t s = 0; s < steps; ++s) {
                if (active) vp8d_reconstruct(p, r, w, mbx, mby, s, lane);
                __syncthreads(); // the next sub-block, the next round (s_work) and the next diagonal read what this one wrote
            }
        }
    }
}

__global__ __launch_bounds__(kVp8dThreads) void vp8dec_filter_kernel(const Vp8DecJob *__restrict__ jobs)
{
    const Vp8DecJob &jb = jobs[blockIdx.x];
    Vp8DecPic p;
    vp8d_pic(p, jb.blob, jb.planes);
    if (!p.filter_type) return; // (uniform over the workgroup)
    const uint32_t slot = threadIdx.x / kVp8dFilterLanes, lane = threadIdx.x % kVp8dFilterLanes;
    constexpr uint32_t kSlots = kVp8dThreads / kVp8dFilterLanes;
    const uint32_t ndiag = p.mbw + 2u * (p.mbh - 1u);
    for (uint32_t d = 0; d < ndiag; ++d) {
        uint32_t lo;
        const uint32_t count = diagonal(p, d, lo);
        for (uint32_t base = 0; base < count; base += kSlots) {
            const bool active = base + slot < count;
            const uint32_t mby = active ? lo + base + slot : 0u, mbx = active ? d - 2u * mby : 0u;
            const Vp8MbRecord &r = p.recs[(uint64_t)mby * p.mbw + mbx];
            for (uint32_t s = 0; s < kVp8dFilterSteps; ++s) {
                if (active) vp8d_filter(p, r, mbx, mby, s, lane);
                __syncthreads();
            }
        }
    }
}

__global__ __launch_bounds__(kVp8dThreads) void vp8dec_alpha_kernel(const Vp8DecJob *__restrict__ jobs)
{
    const Vp8DecJob &jb = jobs[blockIdx.x];
    const Vp8BlobHeader *H = reinterpret_cast<const Vp8BlobHeader *>(jb.blob);
    if (!jb.alpha || !H->alpha) return; // (uniform over the workgroup)
    const uint8_t *in = jb.alpha_src;
    const uint64_t is = jb.alpha_stride;
    uint8_t *out = jb.alpha;
    const uint32_t w = jb.width, h = jb.height, filter = H->alpha_filter, t = threadIdx.x;
    const uint32_t wave = t >> 6, lane = t & 63u;
    if (filter == 0u) {
        for (uint64_t i = t; i < (uint64_t)w * h; i += kVp8dThreads) out[i] = in[i * is];
        return;
    }
    if (filter == 1u || filter == 2u) {
        // a row as prefix sums: its first sample continues the first column (the sum of the first column down to it)
        const uint32_t rows = filter == 1u ? h : 1u;
        for (uint32_t y = wave; y < rows; y += kVp8dWaves) {
            uint32_t c = 0;
            for (uint32_t k = lane; k < y; k += 64u) c += in[(uint64_t)k * w * is];
            uint32_t carry = wave_sum(c);
            for (uint32_t x0 = 0; x0 < w; x0 += 64u) {
                const uint32_t x = x0 + lane;
                uint32_t v = x < w ? in[((uint64_t)y * w + x) * is] : 0u;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t u = __shfl_up(v, o, 64);
                    if (lane >= (uint32_t)o) v += u;
                }
                if (x < w) out[(uint64_t)y * w + x] = (uint8_t)(carry + v);
                carry += __shfl(v, 63, 64);
            }
        }
        if (filter == 1u) return;
        __syncthreads();
        for (uint32_t x = t; x < w; x += kVp8dThreads) { // below the first row: every column on its own
            uint32_t acc = out[x];
            for (uint32_t y = 1; y < h; ++y) { acc += in[((uint64_t)y * w + x) * is]; out[(uint64_t)y * w + x] = (uint8_t)acc; }
        }
        return;
    }
    // gradient: row r of a band of kVp8dThreads rows is thread r's, one sample behind row r - 1
    for (uint32_t b0 = 0; b0 < h; b0 += kVp8dThreads) {
        const uint32_t y = b0 + t;
        for (uint32_t s = 0; s < w + kVp8dThreads - 1u; ++s) {
            if (y < h && s >= t && s - t < w) out[(uint64_t)y * w + (s - t)] = vp8d_alpha_gradient(in[((uint64_t)y * w + (s - t)) * is], out, w, s - t, y);
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kVp8dRgbThreads) void vp8dec_rgb_kernel(const Vp8DecJob *__restrict__ jobs)
{
    const Vp8DecJob &jb = jobs[blockIdx.y];
    const Vp8BlobHeader *H = reinterpret_cast<const Vp8BlobHeader *>(jb.blob);
    const uint64_t npix = (uint64_t)jb.width * jb.height;
    const uint64_t first = ((uint64_t)blockIdx.x * kVp8dRgbThreads + threadIdx.x) * kVp8dRgbRun;
    if (first >= npix) return;
    Vp8DecPic p;
    vp8d_pic(p, jb.blob, jb.planes);
    const uint8_t *alpha = H->alpha ? jb.alpha : nullptr;
    const uint64_t end = first + kVp8dRgbRun < npix ? first + kVp8dRgbRun : npix;
    for (uint64_t i = first; i < end; ++i)
        vp8d_pixel(p, alpha, jb.width, jb.height, jb.channels, (uint32_t)(i % jb.width), (uint32_t)(i / jb.width), jb.dst + i * jb.channels);
}

} // namespace

hipError_t launch_vp8_decode(const Vp8DecJob *jobs, const Vp8DecJob *host_jobs, uint32_t njobs, hipStream_t st, int stage)
{
    if (!njobs) return hipSuccess;
    if (njobs > 65535u) return hipErrorInvalidValue; // (grid.y of the pixel kernel)
    uint32_t nfiltered = 0, nalpha = 0;
    uint64_t max_px = 0;
    for (uint32_t i = 0; i < njobs; ++i) {
        if (host_jobs[i].filtered) { if (nfiltered != i) return hipErrorInvalidValue; ++nfiltered; }
        nalpha += host_jobs[i].alpha != nullptr;
        const uint64_t px = (uint64_t)host_jobs[i].width * host_jobs[i].height;
        if (px > max_px) max_px = px;
    }
    hipLaunchKernelGGL(vp8dec_recon_kernel, dim3(njobs), dim3(kVp8dThreads), 0, st, jobs);
    if (hipError_t e = hipGetLastError()) return e;
    if (stage == 1) return hipSuccess;
    if (nfiltered) {
        hipLaunchKernelGGL(vp8dec_filter_kernel, dim3(nfiltered), dim3(kVp8dThreads), 0, st, jobs);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (stage == 2) return hipSuccess;
    if (nalpha) {
        hipLaunchKernelGGL(vp8dec_alpha_kernel, dim3(njobs), dim3(kVp8dThreads), 0, st, jobs);
        if (hipError_t e = hipGetLastError()) return e;
    }
    const uint64_t per_block = (uint64_t)kVp8dRgbThreads * kVp8dRgbRun;
    hipLaunchKernelGGL(vp8dec_rgb_kernel, dim3((uint32_t)((max_px + per_block - 1u) / per_block), njobs), dim3(kVp8dRgbThreads), 0, st, jobs);
    return hipGetLastError();
}

} // namespace fl
