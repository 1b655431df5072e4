// fl_jpeg_opt.hip -- FLGPU_FEO_JPEG_OPTIMIZE on gfx950: the JPEG encoder of fl_jpeg.hip with per-picture Huffman tables.  Four kernels per
// batch behind one clear of the counts: jpeg_opt_stats_kernel (the transform phase again, the AC symbols counted in LDS), jpeg_opt_tables_kernel
// (fl_jpeg_opt_dev.h, shared with fl_jpeg_420.hip; one workgroup per picture: DC counts, the rule of fl_jpeg_opt_core.h four times, the never-larger decision, the header), then
// jpeg_opt_code_kernel and jpeg_pack_kernel<true>: jpeg_dct_quant_kernel and jpeg_pack_kernel<false> with the tables and the header read from the
// picture's record.
#include "fl_jpeg_dev.h"
#include "fl_jpeg_opt_dev.h"

namespace fl {

namespace {

// The coding launch of a picture with its own tables: jpeg_dct_quant_kernel with the AC tables jpeg_opt_tables_kernel left.
__global__ __launch_bounds__(kJpegThreads) void jpeg_opt_code_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                     uint32_t job_base, const uint32_t *__restrict__ opt)
{
    jpeg_code_units<true>(jobs, arena, job_base, opt);
}

// The grid and the transform phase of jpeg_dct_quant_kernel; then every lane walks its unit's mask as the coder does, but counts the
// (run, size) symbols, ZRL and EOB in the workgroup's LDS histogram (luma, chroma) instead of coding them, and leaves the unit's
// quantised DC term (the DC symbols need the previous block, across wave and workgroup edges: jpeg_opt_tables_kernel counts them).
// The workgroup then adds its used counters to the picture's (hist, cleared before the launch).  Transforming twice costs a second
// pass of the cheap half of jpeg_dct_quant_kernel; keeping the coefficients would cost 128 bytes of scratch per unit.
__global__ __launch_bounds__(kJpegThreads) void jpeg_opt_stats_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                      uint32_t job_base, uint32_t *__restrict__ opt, uint32_t *__restrict__ hist)
{
    __shared__ WaveLds s_w[kWavesPerWg];
    __shared__ uint32_t s_hist[kJpegOptHistWords];
    const JpegJob jb = jobs[job_base + blockIdx.y];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t nblocks = jb.bx * jb.by;
    if (blockIdx.x * kBlocksPerWg >= nblocks) return;    // whole workgroup idle (uniform)
    for (uint32_t i = threadIdx.x; i < kJpegOptHistWords; i += kJpegThreads) s_hist[i] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * kBlocksPerWg + wave * kBlocksPerWave;
    if (first < nblocks) {                               // (wave-uniform; every wave reaches the barrier below)
        const uint32_t count = min(kBlocksPerWave, nblocks - first);
        WaveLds &w = s_w[wave];
        if (jb.c == 4u && (reinterpret_cast<uintptr_t>(jb.src) & 3u) == 0u) transform_blocks<true>(jb, arena, first, count, lane, w);
        else transform_blocks<false>(jb, arena, first, count, lane, w);
        wave_lds_sync();
        uint32_t b, u, u_end;
        bool chroma;
        if constexpr (kBlocksPerWave == 32u) {
            b = lane & 31u;
            chroma = lane >= 32u;
            u = b * 3u + (chroma ? 1u : 0u);
            u_end = b * 3u + (chroma ? 3u : 1u);
        } else {
            b = lane & 15u;
            chroma = lane >= 16u;
            u = b * 3u + (lane >> 4);
            u_end = lane >= 48u ? u : u + 1u;
        }
        if (b >= count) u_end = u;
        uint32_t *h = s_hist + (chroma ? 256u : 0u);
        int16_t *dcs = reinterpret_cast<int16_t *>(opt + jb.opt_off + kJpegOptHeadWords);
        for (; u < u_end; ++u) {
            const int16_t *cf = w.coef[u];
            uint64_t m = w.nz[u];
            dcs[first * 3u + u] = cf[0];
            uint32_t prev = 0;
            while (m) {
                const uint32_t pos = (uint32_t)__builtin_ctzll(m);
                m &= m - 1ull;
                const int32_t cv = cf[pos];
                uint32_t run = pos - prev - 1u;
                prev = pos;
                while (run > 15u) { atomicAdd(&h[0xF0], 1u); run -= 16u; }
                const uint32_t mag = (uint32_t)(cv < 0 ? -cv : cv);
                atomicAdd(&h[(run << 4) | (32u - (uint32_t)__clz(mag))], 1u);
            }
            if (prev != 63u) atomicAdd(&h[0], 1u);
        }
    }
    __syncthreads();
    uint32_t *g = hist + (size_t)blockIdx.y * kJpegOptHistWords;
    for (uint32_t i = threadIdx.x; i < kJpegOptHistWords; i += kJpegThreads) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&g[i], v);
    }
}

} // namespace

hipError_t launch_jpeg_encode_optimized(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_blocks,
                                        uint32_t *opt, uint32_t *hist, bool fallback, hipStream_t st)
{
    if (!njobs || !max_blocks) return hipSuccess;
    const dim3 grid((max_blocks + kBlocksPerWg - 1) / kBlocksPerWg, njobs);
    if (hipError_t e = hipMemsetAsync(hist, 0, (size_t)njobs * kJpegOptHistWords * sizeof(uint32_t), st)) return e;
    hipLaunchKernelGGL(jpeg_opt_stats_kernel, grid, dim3(kJpegThreads), 0, st, jobs, arena, job_base, opt, hist);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_opt_tables_kernel<false>, dim3(njobs), dim3(kOptThreads), 0, st, jobs, arena, job_base, opt, (const uint32_t *)hist, fallback ? 1u : 0u);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_opt_code_kernel, grid, dim3(kJpegThreads), 0, st, jobs, arena, job_base, (const uint32_t *)opt);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pack_kernel<true>, dim3(njobs), dim3(kPackThreads), 0, st, jobs, arena, job_base, (const uint32_t *)opt);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace fl
