// fl_jpeg_opt_dev.h -- jpeg_opt_tables_kernel, the one kernel of FLGPU_FEO_JPEG_OPTIMIZE that fl_jpeg_opt.hip (4:4:4) and fl_jpeg_420.hip
// (FLGPU_FEO_JPEG_420) both launch: a template over the scan's unit order, instantiated once in each translation unit, so that neither
// module holds a kernel the other needs.
#pragma once
#include "fl_jpeg_dev.h"
#include "fl_jpeg_opt_core.h"

namespace fl {

namespace {

constexpr uint32_t kOptThreads = 256; // jpeg_opt_tables_kernel: one workgroup per picture, thread s is symbol s of each table

__device__ __forceinline__ uint32_t std_lut(uint32_t t, uint32_t s) { return (t & 1u) ? kHuff.ac[t >> 1].e[s] : kHuff.dc[t >> 1].e[s]; }

// One workgroup per picture: the DC histograms from the DC terms, then the rule of fl_jpeg_opt_core.h for the four tables (DHT order:
// DC luma, AC luma, DC chroma, AC chroma) -- ranks and places in parallel, thread s for symbol s; the serial part (Moffat-Katajainen,
// the fold) on one thread per table, each in a wave of its own --, the two totals and the decision.  Out: the picture's record
// (fl_jpeg.h) with its own tables and header, or with Annex K's where those are not strictly smaller (or fallback is set).
// k420: the scan's unit order is FLGPU_FEO_JPEG_420's (fl_jpeg_dev.h: unit_is_chroma, unit_dc_back); bx, by count MCUs.
template <bool k420>
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
    const uint32_t tid = threadIdx.x, nunits = jb.bx * jb.by * (k420 ? 6u : 3u);
    uint32_t *rec = opt + jb.opt_off;
    const uint32_t *g = hist + (size_t)blockIdx.x * kJpegOptHistWords;
    s_cnt[0][tid] = 0u; s_cnt[2][tid] = 0u;
    s_cnt[1][tid] = g[tid]; s_cnt[3][tid] = g[256u + tid];
    if (tid < 3u) s_bits[tid] = 0ull;
    __syncthreads();
    const int16_t *dcs = reinterpret_cast<const int16_t *>(rec + kJpegOptHeadWords);
    for (uint32_t u = tid; u < nunits; u += kOptThreads) {   // dc_code's difference and size
        const uint32_t back = unit_dc_back<k420>(u);
        const int32_t diff = (int32_t)dcs[u] - (u >= back ? (int32_t)dcs[u - back] : 0);
        atomicAdd(&s_cnt[unit_is_chroma<k420>(u) ? 2u : 0u][coef_size(diff)], 1u);
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

} // namespace fl
