// fl_blur.hip -- the LDS-tiled separable Gaussian blur in f32: enqueue_launches (fl_batch.cpp) sends a blur group here when the
// window-tile matrix-pipe kernel (fl_wtile.hip) does not take it and every picture's tables fit (add_blur_launch's blur_tiled);
// what is left goes to the generic two passes of fl_resample.hip.
#include <algorithm>
#include <atomic>

#include "fl_blur.h"
#include "fl_kernel_common.h"
#include "fl_kernels.h"

namespace fl {

// ---------------------------------------------------------------------------
// Separable Gaussian blur (image 0.25.6 imageops::blur = the same two-pass machinery with ratio 1 and
// support 2*sigma: 41..81 taps, windows truncated and renormalised at the borders).
//
// One workgroup = one image x a band of BLUR_TY output rows x a tile of <= T - (taps-1) output columns.
//   vertical pass   lane <-> source column (tile + halo).  Every source row of the band's window is loaded
//                   once (u8 -> f32 once) and accumulated into the BLUR_TY output rows in registers; the
//                   weights are wave-uniform (dense [row][BLUR_TY] table staged in LDS, broadcast reads).
//   hand-off        the BLUR_TY unrounded f32 rows go to LDS, lane-contiguous.
//   horizontal pass lane <-> output column.  Neighbouring lanes read neighbouring pixels (ratio 1), so the
//                   LDS reads are conflict free; one weight read feeds BLUR_TY rows x C channels of FMAs.
// BLUR_TY, BLUR_MAXTAPS, the lanes per workgroup (blur_threads) and the LDS bytes are in fl_blur.h, where a host-only
// program can read them too.
// ---------------------------------------------------------------------------

// CS = channels stored per pixel, C = channels filtered.  C < CS only for opaque Rgba8 pictures (every
// letterboxed output of an opaque source): the alpha plane is the constant 255 (any normalised filter
// maps it to 255 again, far from a rounding boundary) and, for a grey picture on a grey fill, R = G = B, so
// one channel is filtered and replicated -- identical arithmetic on identical inputs, bit-identical output.
template <int CS, int C, int TY, int THREADS>
__global__ __launch_bounds__(THREADS) void blur_tile_kernel(const Job *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                        uint32_t job_base)
{
    constexpr int MS = C == 3 ? 4 : C; // floats per pixel in LDS
    constexpr uint32_t T = THREADS;
    // XCD-aware numbering: workgroups are handed to the 8 XCDs round-robin in launch order, and each XCD has its own
    // L2.  The bands of one picture re-read each other's halo rows (41-81 taps against 8 output rows), so all
    // workgroups of a picture are given launch indices that are congruent modulo 8: picture p of every group of 8
    // lives on XCD p % 8 and its halo re-reads hit that L2.
    uint32_t job_i, bid;
    {
        const uint32_t gx = gridDim.x, l = blockIdx.y * gx + blockIdx.x;
        const uint32_t set = l / (8u * gx), m = l - set * 8u * gx;
        const uint32_t inset = min(8u, gridDim.y - set * 8u);
        bid = m / inset;
        job_i = set * 8u + (m - bid * inset);
    }
    const Job jb = jobs[job_base + job_i];
    const uint32_t w = jb.sw, h = jb.sh;
    // one table block per (w, h, sigma): header -> this workgroup's tile and band records -> bulk copies
    const uint32_t *blk = arena + jb.pad0;
    const BlurPlanHeader hd = *reinterpret_cast<const BlurPlanHeader *>(blk);
    const uint32_t nt = hd.nt, htaps = hd.htaps, tw_full = hd.tw_full;
    if (bid >= nt * hd.nb) return;
    const uint32_t band = bid / nt, tile = bid % nt;
    const uint32_t x0 = tile * tw_full, tw = min(tw_full, w - x0);
    const uint32_t y0 = band * TY, ty = min((uint32_t)TY, h - y0);
    const uint32_t tid = threadIdx.x;
    const uint32_t cl = blk[hd.tiles_off + 2 * tile], ncols = blk[hd.tiles_off + 2 * tile + 1]; // ncols <= T by construction
    const uint32_t top = blk[hd.bands_off + 2 * band], nrows = blk[hd.bands_off + 2 * band + 1];

    // LDS: [ wv: rv x TY | mid: TY x blur_midw(T) x MS | wh: htaps x nrows_h (distinct weight vectors) ] -- sized by blur_lds_bytes_of (fl_blur.h)
    float *wv = fl_lds;
    const uint32_t wv_floats = (hd.rv * TY + 3u) & ~3u;
    constexpr uint32_t midw = blur_midw(THREADS); // compile-time row pitch: row offsets fold into the ds_read immediates
    float *mid = fl_lds + wv_floats;
    float *wh = mid + TY * midw * MS;

    {
        const float *vsrc = reinterpret_cast<const float *>(blk + hd.vdense_off) + (size_t)band * hd.rv * TY;
        for (uint32_t i = tid; i < hd.rv * TY; i += T) wv[i] = vsrc[i];
    }
    // columns past the tile's source window are only ever read with zero weights, but must hold finite values
    // (loops are written without integer division: it costs ~40 instructions per element on this ISA)
#pragma unroll
    for (int o = 0; o < TY; ++o)
        for (uint32_t cidx = ncols + tid; cidx < midw; cidx += T) {
#pragma unroll
            for (int c = 0; c < MS; ++c) mid[(o * midw + cidx) * MS + c] = 0.0f;
        }
    // horizontal weights: this column's first tap and the id of its weight vector; the distinct vectors (one for all
    // interior columns, one per column within 2 sigma of a border) are copied tap-major
    const uint32_t *tt = blk + hd.htiles_off + (size_t)tile * (tw_full * 2);
    const uint2 hcol = tid < tw ? *reinterpret_cast<const uint2 *>(tt + 2 * tid) : uint2{0u, 0u};
    const uint32_t hleft = hcol.x, hrow = hcol.y, nrh = hd.nrows_h;
    {
        const float *src = reinterpret_cast<const float *>(blk + hd.hrows_off);
        for (uint32_t i = tid; i < htaps * nrh; i += T) wh[i] = src[i];
    }
    __syncthreads();

    // ---- vertical pass ----
    float acc[TY][C];
#pragma unroll
    for (int o = 0; o < TY; ++o)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[o][c] = 0.0f;
    if (tid < ncols) {
        // raw buffer loads: a pointer read from a descriptor is "generic" to hipcc and would become flat_load,
        // which also counts on lgkmcnt and so serialises against every LDS weight read
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(jb.src), 0, (int)jb.src_bytes, 0x00020000);
        const uint32_t off0 = (top * w + cl + tid) * CS, pitch = w * CS;
        // the image is L2/MALL resident but a load is still ~1 us away: keep PF rows in flight per lane
        constexpr int PF = 12;
        uint32_t ring[PF][CS == 4 ? 1 : C];
        auto fetch = [&](uint32_t r, uint32_t *d) {
            const uint32_t o = off0 + r * pitch; // rows past the image end are range-checked and read 0 (never used)
            if constexpr (CS == 4) d[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0);
            else {
#pragma unroll
                for (int c = 0; c < C; ++c) d[c] = __builtin_amdgcn_raw_buffer_load_b8(rs, o + c, 0, 0);
            }
        };
#pragma unroll
        for (int k = 0; k < PF; ++k) fetch(k, ring[k]);
        for (uint32_t rb = 0; rb < nrows; rb += PF) {
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                const uint32_t r = rb + k;
                float v[C];
                if constexpr (CS == 4) {
                    const uint32_t d = ring[k][0];
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c] = (float)((d >> (8 * c)) & 255u);
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c] = (float)ring[k][c];
                }
                fetch(r + PF, ring[k]);
                if (r < nrows) {
                    f32x4 wq[TY / 4];
#pragma unroll
                    for (int g = 0; g < TY / 4; ++g) wq[g] = *reinterpret_cast<const f32x4 *>(wv + r * TY + 4 * g);
#pragma unroll
                    for (int o = 0; o < TY; ++o) {
                        const f32x4 q4 = wq[o / 4];
                        const float wo = (o & 3) == 0 ? q4.x : (o & 3) == 1 ? q4.y : (o & 3) == 2 ? q4.z : q4.w;
#pragma unroll
                        for (int c = 0; c < C; ++c) acc[o][c] = __builtin_fmaf(v[c], wo, acc[o][c]);
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < TY; ++o) {
            float *m = mid + (o * midw + tid) * MS;
#pragma unroll
            for (int c = 0; c < C; ++c) m[c] = acc[o][c];
        }
    }
    __syncthreads();

    // ---- horizontal pass (tap order: one fused multiply-add per tap) ----
    if (tid < tw) {
#pragma unroll
        for (int o = 0; o < TY; ++o)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[o][c] = 0.0f;
        const float *m0 = mid + hleft * MS;
#pragma unroll 4
        for (uint32_t i = 0; i < htaps; ++i) {
            const float wi = wh[i * nrh + hrow];
#pragma unroll
            for (int o = 0; o < TY; ++o) {
                const float *px = m0 + (o * midw + i) * MS;
                if constexpr (MS == 4) {
                    const f32x4 q = *reinterpret_cast<const f32x4 *>(px);
                    acc[o][0] = __builtin_fmaf(q.x, wi, acc[o][0]);
                    if constexpr (C > 1) acc[o][1] = __builtin_fmaf(q.y, wi, acc[o][1]);
                    if constexpr (C > 2) acc[o][2] = __builtin_fmaf(q.z, wi, acc[o][2]);
                    if constexpr (C > 3) acc[o][3] = __builtin_fmaf(q.w, wi, acc[o][3]);
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[o][c] = __builtin_fmaf(px[c], wi, acc[o][c]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < TY; ++o) {
            if ((uint32_t)o < ty) {
                uint32_t c8[CS];
#pragma unroll
                for (int c = 0; c < C; ++c) c8[c] = round_u8(acc[o][c]);
                if constexpr (CS == 4 && C == 1) { c8[1] = c8[0]; c8[2] = c8[0]; c8[3] = 255u; }
                if constexpr (CS == 4 && C == 3) c8[3] = 255u;
                store_pixel<CS, false>(jb.dst, (y0 + o) * w + x0 + tid, c8, 0u);
            }
        }
    }
}

// host-side sizing and the launch wrapper (called from the host runtime; asynchronous on `st`)

size_t blur_lds_bytes(uint32_t w, uint32_t channels, uint32_t vtaps, uint32_t htaps) { return blur_lds_bytes_of(w, channels, vtaps, htaps); }

uint32_t blur_tile_count(uint32_t w, uint32_t htaps) { return blur_tiles(w, htaps); }
uint32_t blur_lanes(uint32_t w, uint32_t htaps) { return blur_threads(w, htaps); }
uint32_t blur_band_rows(uint32_t channels_filtered) { return (uint32_t)blur_ty(channels_filtered); }

uint32_t blur_grid_x(uint32_t w, uint32_t h, uint32_t htaps, uint32_t channels_filtered)
{
    const uint32_t ty = (uint32_t)blur_ty(channels_filtered);
    return blur_tiles(w, htaps) * ((h + ty - 1) / ty);
}

bool blur_tile_supported(uint32_t htaps) { return htaps >= 1 && htaps <= BLUR_MAXTAPS; }

template <int CS, int C, int THREADS>
static hipError_t launch_blur_tt(const LaunchGeneric &g, uint32_t grid_x, size_t lds, hipStream_t st)
{
    // Ceiling of the kernel's dynamic LDS: add_blur_launch (fl_batch.cpp) marks a group blur_tiled, the condition of this launch,
    // only if blur_lds_bytes() of every picture in it is at most this, and `lds` is their maximum.
    constexpr size_t kBlurLdsMax = 150 * 1024;
    auto k = blur_tile_kernel<CS, C, (C == 1 ? BLUR_TY_MONO : BLUR_TY), THREADS>;
    static std::atomic<uint64_t> attr_set{0}; // the attribute is per function and device: set once per (instantiation, device)
    if (lds > kBlurLdsMax) return hipErrorInvalidValue;
    if (hipError_t e = set_max_lds_once(attr_set, (int)kBlurLdsMax, {reinterpret_cast<const void *>(k)}); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid_x, g.njobs), dim3(THREADS), lds, st, g.jobs, g.arena, g.job_base);
    return hipGetLastError();
}

// g.blur_lanes = lanes per workgroup chosen for the group (blur_threads of its pictures)
template <int CS, int C>
static hipError_t launch_blur_t(const LaunchGeneric &g, uint32_t grid_x, size_t lds, hipStream_t st)
{
    switch (g.blur_lanes) {
    case 256: return launch_blur_tt<CS, C, 256>(g, grid_x, lds, st);
    case 384: return launch_blur_tt<CS, C, 384>(g, grid_x, lds, st);
    case 512: return launch_blur_tt<CS, C, 512>(g, grid_x, lds, st);
    }
    return hipErrorInvalidValue;
}

// g.cs = channels stored, g.pre = channels filtered (see blur_tile_kernel)
hipError_t launch_blur_tile(const LaunchGeneric &g, uint32_t grid_x, size_t lds, hipStream_t st)
{
    if (g.cs == 4 && g.pre == 1) return launch_blur_t<4, 1>(g, grid_x, lds, st);
    if (g.cs == 4 && g.pre == 3) return launch_blur_t<4, 3>(g, grid_x, lds, st);
    switch (g.cs) {
    case 1: return launch_blur_t<1, 1>(g, grid_x, lds, st);
    case 2: return launch_blur_t<2, 2>(g, grid_x, lds, st);
    case 3: return launch_blur_t<3, 3>(g, grid_x, lds, st);
    case 4: return launch_blur_t<4, 4>(g, grid_x, lds, st);
    }
    return hipErrorInvalidValue;
}

} // namespace fl
