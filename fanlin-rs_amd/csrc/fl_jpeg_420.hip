// fl_jpeg_420.hip -- FLGPU_FEO_JPEG_420 on gfx950: the JPEG encoder of fl_jpeg.hip with Cb and Cr halved in both directions.  The scan is
// one interleaved baseline scan of 16 x 16 MCUs, six units each: Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr.  Samples, transform, quantiser, coder,
// packer and header are fl_jpeg.hip's; what differs is where a lane's pixels lie, the 2 x 2 average in front of the chroma transform,
// which code table a unit takes and where its DC predecessor sits (fl_jpeg_dev.h: unit_is_chroma, unit_dc_back).
//
//   jpeg420_dct_quant_kernel   one wave per 8 consecutive MCUs = 48 units, in the two phases of jpeg_dct_quant_kernel.  Transform, MCU after
//                              MCU: lane (r, c) holds pixel (r, c) of each of the four Y blocks; their transforms run interleaved, as the
//                              three components of a block do in fl_jpeg.hip.  Every lane leaves the Cb and Cr bytes of its four pixels
//                              in a 16 x 16 LDS tile, lane (r, c) then sums the bytes at (2r..2r+1, 2c..2c+1) -- pixels are clamped to the
//                              picture when they are loaded, so replicated edge pixels take part in the average -- and one more
//                              interleaved step transforms Cb and Cr.  Coding: lane l codes unit l (MCU l / 6, slot l % 6; lanes 48-63 idle).
//   jpeg_pack_kernel<.., true> fl_jpeg_dev.h's pack kernel with this unit order.
// With FLGPU_FEO_JPEG_OPTIMIZE as well: jpeg420_opt_stats_kernel, jpeg_opt_tables_kernel<true> (fl_jpeg_opt_dev.h), jpeg420_opt_code_kernel,
// jpeg_pack_kernel<true, true> -- fl_jpeg_opt.hip's sequence over this scan.
// A translation unit of its own for the reason fl_jpeg_opt.hip is one: the modules of the kernels that existed before hold what they held,
// and their instruction streams are unchanged (profiles/pr_jpeg_420.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_jpeg_dev.h"
#include "fl_jpeg_opt_dev.h"

namespace fl {

namespace {

constexpr uint32_t kMcuUnits = 6;
constexpr uint32_t kMcusPerWave = 8;
constexpr uint32_t kMcusPerWg = kWavesPerWg * kMcusPerWave;
constexpr uint32_t kUnitsPerWave420 = kMcuUnits * kMcusPerWave;
static_assert(kUnitsPerWave420 <= 64u, "the coding phase: one lane per unit");

// WaveLds of fl_jpeg_dev.h with exchange buffers for four interleaved transforms, and the MCU's chroma bytes.
struct WaveLds420 {
    int16_t coef[kUnitsPerWave420][64];
    uint64_t nz[kUnitsPerWave420];                       // bit k: zig-zag coefficient k (k >= 1) is not zero
    __attribute__((aligned(16))) int16_t smp[4][64];     // samples, natural order
    __attribute__((aligned(16))) int16_t p1[4][64];      // pass-1 results, transposed
    __attribute__((aligned(4))) uint16_t cbcr[16][16];   // Cb | Cr << 8 of every pixel of the MCU
};

// Block k (0..3: (0,0) (0,1) (1,0) (1,1)) of MCU (mrow, mcol): its pixel (r, c), clamped to the picture as block_pixel clamps.
template <bool kRgba>
__device__ __forceinline__ uint32_t mcu_pixel(const JpegJob &jb, uint32_t mrow, uint32_t mcol, uint32_t k, uint32_t r, uint32_t c)
{
    uint32_t px = mcol * 16u + (k & 1u) * 8u + c, py = mrow * 16u + (k >> 1) * 8u + r;
    px = px < jb.w ? px : jb.w - 1u;
    py = py < jb.h ? py : jb.h - 1u;
    if constexpr (kRgba) return ((const __attribute__((address_space(1))) uint32_t *)jb.src)[(size_t)py * jb.w + px];
    uint32_t pr, pg, pb, pa;
    load_rgba(jb.src + ((size_t)py * jb.w + px) * jb.c, jb.c, pr, pg, pb, pa);
    return pr | (pg << 8) | (pb << 16);
}

// dct_quant_block for N units that share a quantisation table (four Y blocks, or Cb and Cr): the same two passes, interleaved.
template <int N>
__device__ __forceinline__ void dct_quant_units(const uint32_t (&smp)[N], uint32_t nat, uint32_t r, uint32_t c, const uint32_t (&m1)[4],
                                                const uint32_t (&m2)[4], uint4 k1, uint32_t q, uint32_t magic, WaveLds420 &w, int32_t (&qv)[N])
{
#pragma unroll
    for (int k = 0; k < N; ++k) w.smp[k][nat] = (int16_t)smp[k];
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int32_t p = dot8_i16(m1, *reinterpret_cast<const uint4 *>(w.smp[k] + r * 8));
        const int32_t v1 = ((p << k1.x) + (int32_t)k1.y) >> 11;
        w.p1[k][c * 8 + r] = (int16_t)v1;
    }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int32_t p2 = dot8_i16(m2, *reinterpret_cast<const uint4 *>(w.p1[k] + c * 8));
        const int32_t d = (p2 + (int32_t)k1.z) >> k1.w;
        const int32_t sg = d >> 31;
        const uint32_t an = (uint32_t)((d ^ sg) - sg) >> 3;
        const uint32_t rq = __umulhi(2u * an + q, magic);
        qv[k] = ((int32_t)rq ^ sg) - sg;
    }
}

// The quantised DC term of a unit of one value s (transform_blocks says why); q, magic: those of natural index 0.
__device__ __forceinline__ int16_t flat_dc(uint32_t s, uint32_t q, uint32_t magic)
{
    const int32_t d = 64 * ((int32_t)s - 128);
    const int32_t sg = d >> 31;
    const uint32_t an = (uint32_t)((d ^ sg) - sg) >> 3;
    const uint32_t rq = __umulhi(2u * an + q, magic);
    return (int16_t)(((int32_t)rq ^ sg) - sg);
}

__device__ __forceinline__ bool wave_uniform(uint32_t v) { return __ballot(v != (uint32_t)__builtin_amdgcn_readfirstlane((int)v)) == 0ull; }

// The transform phase: MCUs first .. first + count - 1 into the wave's LDS, unit 6 i + slot.
template <bool kRgba>
__device__ __forceinline__ void transform_mcus(const JpegJob &jb, const uint32_t *__restrict__ arena, uint32_t first, uint32_t count,
                                               uint32_t lane, WaveLds420 &w)
{
    const uint32_t nat = kNatural.n[lane], r = nat >> 3, c = nat & 7u;
    uint32_t m1[4], m2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m1[j] = pack_i16(kFdct.a[c][2 * j], kFdct.a[c][2 * j + 1]);
        m2[j] = pack_i16(kFdct.a[r][2 * j], kFdct.a[r][2 * j + 1]);
    }
    const uint8_t *qt = reinterpret_cast<const uint8_t *>(arena + jb.tab_off) + 624;
    const uint32_t *mg = reinterpret_cast<const uint32_t *>(qt + 128);
    const uint32_t ql = qt[nat], qc = qt[64 + nat], magl = mg[nat], magc = mg[64 + nat];
    const uint4 k1 = {(c == 0u || c == 4u) ? 13u : 0u, c == 0u ? (uint32_t)(-(8 * 128) * 8192) : (c == 4u ? 0u : 1u << 10),
                      (r == 0u || r == 4u) ? 2u : 1u << 14, (r == 0u || r == 4u) ? 2u : 15u};
    uint32_t mrow = first / jb.bx, mcol = first - mrow * jb.bx;
    // the four pixels of the next MCU are in flight while an MCU is transformed (mcu_pixel clamps: no condition on the loads)
    uint32_t ahead[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) ahead[k] = mcu_pixel<kRgba>(jb, mrow, mcol, k, r, c);
    if (++mcol == jb.bx) { mcol = 0; ++mrow; }
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t y[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t rgb = kRgba ? ahead[k] & 0xffffffu : ahead[k];
            ahead[k] = mcu_pixel<kRgba>(jb, mrow, mcol, k, r, c);
            uint32_t cb, cr;
            jfif_px(rgb, y[k], cb, cr);
            w.cbcr[(k >> 1) * 8u + r][(k & 1u) * 8u + c] = (uint16_t)(cb | (cr << 8));
        }
        if (++mcol == jb.bx) { mcol = 0; ++mrow; }
        const uint32_t u0 = i * kMcuUnits;
        // the one-colour shortcut of transform_blocks, for the four Y blocks together (each with its own value) ...
        if (wave_uniform(y[0]) && wave_uniform(y[1]) && wave_uniform(y[2]) && wave_uniform(y[3])) {
            if (lane == 0u) {
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) { w.coef[u0 + k][0] = flat_dc(y[k], ql, magl); w.nz[u0 + k] = 0ull; }
            }
        } else {
            int32_t qv[4];
            dct_quant_units<4>(y, nat, r, c, m1, m2, k1, ql, magl, w, qv);
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                w.coef[u0 + k][lane] = (int16_t)qv[k];
                const uint64_t nz = __ballot(qv[k] != 0) & ~1ull;
                if (lane == 0u) w.nz[u0 + k] = nz;
            }
        }
        wave_lds_sync();
        // the 2 x 2 average: (c00 + c01 + c10 + c11 + 2) >> 2 on the bytes; a dword holds the two pixels of a row
        const uint32_t a = *reinterpret_cast<const uint32_t *>(&w.cbcr[2u * r][2u * c]);
        const uint32_t b = *reinterpret_cast<const uint32_t *>(&w.cbcr[2u * r + 1u][2u * c]);
        wave_lds_sync();                                  // (the next MCU's bytes are written behind these reads)
        const uint32_t ch[2] = {((a & 255u) + ((a >> 16) & 255u) + (b & 255u) + ((b >> 16) & 255u) + 2u) >> 2,
                                (((a >> 8) & 255u) + (a >> 24) + ((b >> 8) & 255u) + (b >> 24) + 2u) >> 2};
        // ... and for Cb and Cr, judged on the averaged samples: four flat Y blocks of different colours have a chroma block that is not flat
        if (wave_uniform(ch[0]) && wave_uniform(ch[1])) {
            if (lane == 0u) {
#pragma unroll
                for (uint32_t k = 0; k < 2u; ++k) { w.coef[u0 + 4u + k][0] = flat_dc(ch[k], qc, magc); w.nz[u0 + 4u + k] = 0ull; }
            }
            continue;
        }
        int32_t qv[2];
        dct_quant_units<2>(ch, nat, r, c, m1, m2, k1, qc, magc, w, qv);
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k) {
            w.coef[u0 + 4u + k][lane] = (int16_t)qv[k];
            const uint64_t nz = __ballot(qv[k] != 0) & ~1ull;
            if (lane == 0u) w.nz[u0 + 4u + k] = nz;
        }
    }
}

template <bool kOwn>
__device__ __forceinline__ void jpeg420_code_units(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena, uint32_t job_base,
                                                   const uint32_t *__restrict__ opt)
{
    __shared__ WaveLds420 s_w[kWavesPerWg];
    __shared__ uint32_t s_ac[512];                       // AC code tables (luma, chroma)
    const JpegJob jb = jobs[job_base + blockIdx.y];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t nmcus = jb.bx * jb.by;
    if (blockIdx.x * kMcusPerWg >= nmcus) return;        // whole workgroup idle (uniform)
    if constexpr (kOwn) stage_ac_luts(s_ac, opt + jb.opt_off + kJpegOptAcLut);
    else stage_ac_luts(s_ac);
    const uint32_t first = blockIdx.x * kMcusPerWg + wave * kMcusPerWave;
    if (first >= nmcus) return;                          // wave-uniform; from here on waves never synchronise with each other
    const uint32_t count = min(kMcusPerWave, nmcus - first);
    WaveLds420 &w = s_w[wave];

    if (jb.c == 4u && (reinterpret_cast<uintptr_t>(jb.src) & 3u) == 0u) transform_mcus<true>(jb, arena, first, count, lane, w);
    else transform_mcus<false>(jb, arena, first, count, lane, w);
    wave_lds_sync();

    // ---- coding phase: lane l codes unit l of the wave (jpeg_code_units' walk) ----
    const uint32_t mcu = lane / kMcuUnits, slot = lane - mcu * kMcuUnits;
    if (mcu >= count) return;                            // (lanes 48-63: mcu >= 8 >= count)
    const uint32_t *tab = s_ac + (slot >= 4u ? 256u : 0u);
    const uint32_t eob = tab[0], zrl = tab[0xF0];
    const uint32_t unit = first * kMcuUnits + lane;
    const int16_t *cf = w.coef[lane];
    uint64_t m = w.nz[lane];
    UnitBits ub{0ull, 0u, 0u, 0u, (global_u32 *)jb.acbits + (size_t)unit * kAcWordsPerUnit, 0u, 0u, 0u};
    uint32_t prev = 0;
    uint32_t pos = (uint32_t)__builtin_ctzll(m | (1ull << 63));
    int32_t v = cf[pos];
    while (m) {
        const uint32_t cpos = pos;
        const int32_t cv = v;
        m &= m - 1ull;
        pos = (uint32_t)__builtin_ctzll(m | (1ull << 63));
        v = cf[pos];
        uint32_t run = cpos - prev - 1u;
        prev = cpos;
        while (run > 15u) { ub.put(zrl & 0xffffu, zrl >> 16); run -= 16u; }
        const uint32_t mag = (uint32_t)(cv < 0 ? -cv : cv);
        const uint32_t size = 32u - (uint32_t)__clz(mag);
        const uint32_t value = (uint32_t)(cv + (cv >> 31)) & ((1u << size) - 1u);
        const uint32_t e = tab[(run << 4) | size];
        ub.put(((e & 0xffffu) << size) | value, (e >> 16) + size);
    }
    if (prev != 63u) ub.put(eob & 0xffffu, eob >> 16);
    if (ub.pend) ub.word((uint32_t)(ub.acc << (32u - ub.pend)));
    const u32x4 rec = {((uint32_t)(uint16_t)cf[0]) | (ub.total << 16), ub.w0, ub.w1, ub.w2};
    ((global_u32x4 *)jb.units)[unit] = rec;
}

__global__ __launch_bounds__(kJpegThreads) void jpeg420_dct_quant_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                         uint32_t job_base)
{
    jpeg420_code_units<false>(jobs, arena, job_base, nullptr);
}

__global__ __launch_bounds__(kJpegThreads) void jpeg420_opt_code_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                        uint32_t job_base, const uint32_t *__restrict__ opt)
{
    jpeg420_code_units<true>(jobs, arena, job_base, opt);
}

// jpeg_opt_stats_kernel over this scan: the same grid and transform phase as jpeg420_dct_quant_kernel, then lane l counts unit l's symbols.
__global__ __launch_bounds__(kJpegThreads) void jpeg420_opt_stats_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                         uint32_t job_base, uint32_t *__restrict__ opt, uint32_t *__restrict__ hist)
{
    __shared__ WaveLds420 s_w[kWavesPerWg];
    __shared__ uint32_t s_hist[kJpegOptHistWords];
    const JpegJob jb = jobs[job_base + blockIdx.y];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t nmcus = jb.bx * jb.by;
    if (blockIdx.x * kMcusPerWg >= nmcus) return;        // whole workgroup idle (uniform)
    for (uint32_t i = threadIdx.x; i < kJpegOptHistWords; i += kJpegThreads) s_hist[i] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * kMcusPerWg + wave * kMcusPerWave;
    if (first < nmcus) {                                 // (wave-uniform; every wave reaches the barrier below)
        const uint32_t count = min(kMcusPerWave, nmcus - first);
        WaveLds420 &w = s_w[wave];
        if (jb.c == 4u && (reinterpret_cast<uintptr_t>(jb.src) & 3u) == 0u) transform_mcus<true>(jb, arena, first, count, lane, w);
        else transform_mcus<false>(jb, arena, first, count, lane, w);
        wave_lds_sync();
        const uint32_t mcu = lane / kMcuUnits, slot = lane - mcu * kMcuUnits;
        if (mcu < count) {
            uint32_t *h = s_hist + (slot >= 4u ? 256u : 0u);
            int16_t *dcs = reinterpret_cast<int16_t *>(opt + jb.opt_off + kJpegOptHeadWords);
            const int16_t *cf = w.coef[lane];
            uint64_t m = w.nz[lane];
            dcs[first * kMcuUnits + lane] = cf[0];
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

hipError_t launch_jpeg_encode_420(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_mcus, hipStream_t st)
{
    if (!njobs || !max_mcus) return hipSuccess;
    hipLaunchKernelGGL(jpeg420_dct_quant_kernel, dim3((max_mcus + kMcusPerWg - 1) / kMcusPerWg, njobs), dim3(kJpegThreads), 0, st, jobs, arena, job_base);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL((jpeg_pack_kernel<false, true>), dim3(njobs), dim3(kPackThreads), 0, st, jobs, arena, job_base, (const uint32_t *)nullptr);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_jpeg_encode_420_optimized(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_mcus,
                                            uint32_t *opt, uint32_t *hist, bool fallback, hipStream_t st)
{
    if (!njobs || !max_mcus) return hipSuccess;
    const dim3 grid((max_mcus + kMcusPerWg - 1) / kMcusPerWg, njobs);
    if (hipError_t e = hipMemsetAsync(hist, 0, (size_t)njobs * kJpegOptHistWords * sizeof(uint32_t), st)) return e;
    hipLaunchKernelGGL(jpeg420_opt_stats_kernel, grid, dim3(kJpegThreads), 0, st, jobs, arena, job_base, opt, hist);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_opt_tables_kernel<true>, dim3(njobs), dim3(kOptThreads), 0, st, jobs, arena, job_base, opt, (const uint32_t *)hist, fallback ? 1u : 0u);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg420_opt_code_kernel, grid, dim3(kJpegThreads), 0, st, jobs, arena, job_base, (const uint32_t *)opt);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL((jpeg_pack_kernel<true, true>), dim3(njobs), dim3(kPackThreads), 0, st, jobs, arena, job_base, (const uint32_t *)opt);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace fl
