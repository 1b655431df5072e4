// fl_jpeg_opt.hip -- FLGPU_FEO_JPEG_OPTIMIZE on gfx950: the JPEG encoder of fl_jpeg.hip with per-picture Huffman tables.  Four kernels per
// batch behind one clear of the counts: jpeg_opt_stats_kernel (the transform phase again, the AC symbols counted in LDS), jpeg_opt_tables_kernel
// (one workgroup per picture: DC counts, the rule of fl_jpeg_opt_core.h four times, the never-larger decision, the header), then
// jpeg_opt_code_kernel and jpeg_pack_kernel<true>: jpeg_dct_quant_kernel and jpeg_pack_kernel<false> with the tables and the header read from the
// picture's record.
#include "fl_jpeg_dev.h"
#include "fl_jpeg_opt_core.h"

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

constexpr uint32_t kOptThreads = 256; // jpeg_opt_tables_kernel: one workgroup per picture, thread s is symbol s of each table

__device__ __forceinline__ uint32_t std_lut(uint32_t t, uint32_t s) { return (t & 1u) ? kHuff.ac[t >> 1].e[s] : kHuff.dc[t >> 1].e[s]; }

// One workgroup per picture: the DC histograms from the DC terms, then the rule of fl_jpeg_opt_core.h for the four tables (DHT order:
// DC luma, AC luma, DC chroma, AC chroma) -- ranks and places in parallel, thread s for symbol s; the serial part (Moffat-Katajainen,
// the fold) on one thread per table, each in a wave of its own --, the two totals and the decision.  Out: the picture's record
// (fl_jpeg.h) with its own tables and header, or with Annex K's where those are not strictly smaller (or fallback is set).
__global__ __launch_bounds__(kOptThreads) void jpeg_opt_tables_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                      uint32_t job_base, uint32_t *__restrict__ opt,
                                                                      const uint32_t *__restrict__ hist, uint32_t fallback)
{
    __shared__ uint32_t s_cnt[4][256];
    __shared__ uint32_t s_A[4][kJpegOptMaxLeaves + 1u];
    __shared__ JpegOptCode s_code[4];
    __shared__ uint8_t s_len[4][256], s_vals[4][256];
    __shared__ unsigned long long s_bits[3];             // code bits with the picture's tables, with Annex K's; value bits
    __shared__ uint32_t s_used[4];
    const JpegJob jb = jobs[job_base + blockIdx.x];
    const uint32_t tid = threadIdx.x, nunits = jb.bx * jb.by * 3u;
    uint32_t *rec = opt + jb.opt_off;
    const uint32_t *g = hist + (size_t)blockIdx.x * kJpegOptHistWords;
    s_cnt[0][tid] = 0u; s_cnt[2][tid] = 0u;
    s_cnt[1][tid] = g[tid]; s_cnt[3][tid] = g[256u + tid];
    if (tid < 3u) s_bits[tid] = 0ull;
    __syncthreads();
    const int16_t *dcs = reinterpret_cast<const int16_t *>(rec + kJpegOptHeadWords);
    for (uint32_t u = tid; u < nunits; u += kOptThreads) {   // dc_code's difference and size
        const int32_t diff = (int32_t)dcs[u] - (u >= 3u ? (int32_t)dcs[u - 3u] : 0);
        atomicAdd(&s_cnt[(u % 3u) ? 2u : 0u][coef_size(diff)], 1u);
    }
    __syncthreads();
    uint32_t rank[4];
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t) {
        uint32_t used;
        rank[t] = jpeg_opt_rank(s_cnt[t], tid, &used);
        if (s_cnt[t][tid]) s_A[t][1u + rank[t]] = s_cnt[t][tid];
        if (tid == 0u) { s_used[t] = used; s_A[t][0] = 1u; }
    }
    __syncthreads();
    if ((tid & 63u) == 0u) jpeg_opt_lengths(s_A[tid >> 6], (int)s_used[tid >> 6] + 1, s_code[tid >> 6]);
    __syncthreads();
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t) s_len[t][tid] = s_cnt[t][tid] ? (uint8_t)jpeg_opt_length_of_rank(s_code[t].num, rank[t]) : (uint8_t)0;
    __syncthreads();
    uint32_t lut[4];
    unsigned long long own = 0, std_bits = 0, val = 0;
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t) {
        const uint32_t l = s_len[t][tid], n = s_cnt[t][tid];
        lut[t] = 0u;
        if (l) {
            const uint32_t pos = jpeg_opt_pos(s_len[t], tid);
            lut[t] = (l << 16) | (s_code[t].first_code[l] + pos);
            s_vals[t][s_code[t].first_idx[l] + pos] = (uint8_t)tid;
            own += (unsigned long long)n * l;
            std_bits += (unsigned long long)n * (std_lut(t, tid) >> 16);
            val += (unsigned long long)n * jpeg_opt_value_bits(t, tid);
        }
    }
    if (own) { atomicAdd(&s_bits[0], own); atomicAdd(&s_bits[1], std_bits); }
    if (val) atomicAdd(&s_bits[2], val);
    __syncthreads();
    const uint32_t used[4] = {s_used[0], s_used[1], s_used[2], s_used[3]};
    const uint32_t own_header = jpeg_opt_header_bytes(used);
    const bool on = jpeg_opt_decide(own_header, s_bits[0], s_bits[1], s_bits[2], fallback != 0u);
    if (tid == 0u) { rec[kJpegOptHdrLen] = on ? own_header : kJpegHeaderBytes; rec[kJpegOptFlag] = on ? 1u : 0u; }
    if (tid < kDcCodes) {
        rec[kJpegOptDcLut + tid] = on ? lut[0] : std_lut(0, tid);
        rec[kJpegOptDcLut + kDcCodes + tid] = on ? lut[2] : std_lut(2, tid);
    }
    rec[kJpegOptAcLut + tid] = on ? lut[1] : std_lut(1, tid);
    rec[kJpegOptAcLut + 256u + tid] = on ? lut[3] : std_lut(3, tid);
    const uint8_t *hdr = reinterpret_cast<const uint8_t *>(arena + jb.tab_off);
    uint8_t *out = reinterpret_cast<uint8_t *>(rec + kJpegOptHeader);
    if (!on) {
        for (uint32_t i = tid; i < kJpegHeaderBytes; i += kOptThreads) out[i] = hdr[i];
        return;
    }
    if (tid < kJpegOptPrefixBytes) out[tid] = hdr[tid];
    uint32_t at = kJpegOptPrefixBytes;
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t) {
        if (tid < kJpegOptDhtHead) out[at + tid] = jpeg_opt_dht_head(t, tid, s_code[t].num, used[t]);
        if (tid < used[t]) out[at + kJpegOptDhtHead + tid] = s_vals[t][tid];
        at += kJpegOptDhtHead + used[t];
    }
    if (tid < kJpegOptSosBytes) out[at + tid] = hdr[kJpegHeaderBytes - kJpegOptSosBytes + tid];
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
    hipLaunchKernelGGL(jpeg_opt_tables_kernel, dim3(njobs), dim3(kOptThreads), 0, st, jobs, arena, job_base, opt, (const uint32_t *)hist, fallback ? 1u : 0u);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_opt_code_kernel, grid, dim3(kJpegThreads), 0, st, jobs, arena, job_base, (const uint32_t *)opt);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pack_kernel<true>, dim3(njobs), dim3(kPackThreads), 0, st, jobs, arena, job_base, (const uint32_t *)opt);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace fl
