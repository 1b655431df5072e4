// fl_resample.hip -- the f32 two-pass resamplers: what route_resample (fl_batch.cpp) has left when neither the matrix-pipe kernels
// (fl_mfma.hip, fl_wtile.hip) nor the streaming kernel (fl_stream.hip) take a picture -- grayscale pre-ops at mild ratios, geometries
// those planners refuse, everything under the debug switches that turn them off.
//   resample_tile_kernel                          both passes through an LDS tile (S1_TILE: try_tile, if a tile width fits).
//   vpass_generic_kernel + hpass_generic_kernel   the same passes through an f32 intermediate in HBM (S1_GENERIC: tile widths the
//                                                 LDS cannot hold, DBG_NO_TILE), and enqueue_launches' fallback for a blur group
//                                                 that neither fl_wtile.hip nor fl_blur.hip serves.
#include <algorithm>
#include <atomic>

#include "fl_kernel_common.h"
#include "fl_kernels.h"

namespace fl {

// ---------------------------------------------------------------------------
// Generic two-pass resample (any ratio, any size): vertical pass into an f32
// intermediate in HBM, horizontal pass out of it.  Used for up-scaling, for
// Gaussian blur (same machinery, ratio 1) and as the fallback of the fused
// streaming kernel.  Output-stationary: one thread per output sample.
// ---------------------------------------------------------------------------

template <int CS, int PRE>
__global__ __launch_bounds__(256) void vpass_generic_kernel(const Job *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                            float *__restrict__ mid, uint32_t job_base)
{
    constexpr int MC = mid_channels(CS, PRE);
    const Job jb = jobs[job_base + blockIdx.y];
    // flat over rows x columns of THIS job: narrow pictures (thumbnails) still fill their waves
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= jb.rh * jb.sw) return;
    const uint32_t oy = idx / jb.sw, x = idx - oy * jb.sw;
    const AxisTable *tab = reinterpret_cast<const AxisTable *>(arena + jb.vtab);
    const uint32_t left = arena[tab->left_off + oy];
    const uint32_t n = arena[tab->count_off + oy];
    const float *w = reinterpret_cast<const float *>(arena + tab->weights_off + arena[tab->woff_off + oy]);
    float acc[MC];
#pragma unroll
    for (int k = 0; k < MC; ++k) acc[k] = 0.0f;
    const uint8_t *p = jb.src + ((size_t)left * jb.sw + x) * CS;
    const size_t pitch = (size_t)jb.sw * CS;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t s[CS];
#pragma unroll
        for (int k = 0; k < CS; ++k) s[k] = p[k];
        float v[MC > CS ? MC : CS];
        preop_pixel<CS, PRE>(s, v);
        const float wi = w[i];
#pragma unroll
        for (int k = 0; k < MC; ++k) acc[k] = __builtin_fmaf(v[k], wi, acc[k]);
        p += pitch;
    }
    float *o = mid + (size_t)jb.mid_off + ((size_t)oy * jb.sw + x) * MC;
#pragma unroll
    for (int k = 0; k < MC; ++k) o[k] = acc[k];
}

template <int MC, bool LB, bool GROUPED>
__global__ __launch_bounds__(256) void hpass_generic_kernel(const Job *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                            const float *__restrict__ mid, uint32_t job_base)
{
    const Job jb = jobs[job_base + blockIdx.y];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;  // flat over the kept (cropped) window of this job
    if (idx >= jb.ch * jb.cw) return;
    const uint32_t yy = idx / jb.cw, xx = idx - yy * jb.cw; // row / column inside the kept window
    const uint32_t x = jb.cx + xx, y = jb.cy + yy;
    const AxisTable *tab = reinterpret_cast<const AxisTable *>(arena + jb.htab);
    const uint32_t left = arena[tab->left_off + x];
    const uint32_t n = arena[tab->count_off + x];
    const float *w = reinterpret_cast<const float *>(arena + tab->weights_off + arena[tab->woff_off + x]);
    const float *p = mid + (size_t)jb.mid_off + ((size_t)y * jb.sw + left) * MC;
    // Horizontal summation order (also the oracle's FO_ARITH_FMA mode).  Lanczos3 resize (GROUPED): taps are
    // grouped by aligned blocks of 4 source pixels; inside a block one fused multiply-add per tap in
    // ascending order starting from 0, then the block sums are added in ascending order.  Gaussian blur:
    // one fused multiply-add per tap in tap order.
    float acc[MC], part[MC];
#pragma unroll
    for (int k = 0; k < MC; ++k) { acc[k] = 0.0f; part[k] = 0.0f; }
    for (uint32_t i = 0; i < n; ++i) {
        if (GROUPED && i != 0 && ((left + i) & 3u) == 0u) {
#pragma unroll
            for (int k = 0; k < MC; ++k) { acc[k] = acc[k] + part[k]; part[k] = 0.0f; }
        }
        const float wi = w[i];
#pragma unroll
        for (int k = 0; k < MC; ++k) part[k] = __builtin_fmaf(p[k], wi, part[k]);
        p += MC;
    }
#pragma unroll
    for (int k = 0; k < MC; ++k) acc[k] = acc[k] + part[k];
    uint32_t c[MC];
#pragma unroll
    for (int k = 0; k < MC; ++k) c[k] = round_u8(acc[k]);
    store_pixel<MC, LB>(jb.dst, (jb.oy + yy) * jb.dw + jb.ox + xx, c, jb.fill);
}

// ---------------------------------------------------------------------------
// Tiled two-pass resample (round 3): the generic path without its f32 intermediate in HBM.  One workgroup = one picture x
// one tile of kTileRows output rows x jb.pad1 output columns (a power of two the host chose so that the tile's source
// column window fits the LDS budget).  Vertical pass: wave w takes output rows w, w + 4, ...; lanes walk the window's
// source columns (coalesced byte loads, weights wave-uniform) and leave the unrounded f32 sums in LDS.  Horizontal pass:
// one thread per output pixel reads its taps from that LDS tile.  The arithmetic is the generic kernels' -- one fused
// multiply-add per tap in tap order vertically; horizontally Lanczos3 taps grouped by aligned blocks of 4 source pixels with
// the block sums added in ascending order (GROUPED, also the oracle's ARITH_FMA mode), Gaussian taps in tap order -- so the
// results are bit-identical to them.  Serves what neither the matrix-pipe nor the streaming kernel takes: up-scales, mild
// down-scales, odd pitches (image 0.25.6 imageops/sample.rs vertical_sample + horizontal_sample).
// ---------------------------------------------------------------------------
constexpr uint32_t kTileRows = 8; // (16 rows and 64 KB of LDS per workgroup left two workgroups per CU, and the kernel waited on its own loads)
constexpr uint32_t kTilePrefetch = 14; // source rows in flight per thread in the vertical pass (ratio 1: a band touches 14 rows)
typedef uint32_t __attribute__((aligned(1))) u32_unaligned; // (gfx950 loads a dword from any byte address: one global_load_dword)

template <int CS, int PRE, bool LB, bool GROUPED>
__global__ __launch_bounds__(256) void resample_tile_kernel(const Job *__restrict__ jobs, const uint32_t *__restrict__ arena, uint32_t job_base,
                                                            uint32_t nbands)
{
    extern __shared__ float tile_mid[]; // [rows of the tile][source columns of its window][MC], then the horizontal weights of the tile's columns
    constexpr int MC = mid_channels(CS, PRE);
    const Job jb = jobs[job_base + blockIdx.y];
    const uint32_t tw = jb.pad1, tw_log = 31u - (uint32_t)__clz(tw);
    const uint32_t tiles_x = (jb.cw + tw - 1u) >> tw_log;
    if (blockIdx.x >= tiles_x * nbands) return;
    // One workgroup = one COLUMN of tiles (x range) of one band of rows: everything the horizontal pass needs -- the window's
    // first source column, its weights (staged in LDS), every thread's own (left, count, weight offset) -- is fetched once and
    // serves all tiles of the column; what is left per tile are the row tables of the vertical pass.  (A workgroup per tile spent
    // most of its 23 us in these chains of dependent table loads.)
    const uint32_t band = blockIdx.x / tiles_x, tx = blockIdx.x - band * tiles_x;
    const uint32_t band_rows = ((jb.ch + nbands - 1u) / nbands + kTileRows - 1u) / kTileRows * kTileRows;
    const uint32_t yb0 = jb.cy + band * band_rows, yb1 = min(yb0 + band_rows, jb.cy + jb.ch);
    if (yb0 >= yb1) return;
    const uint32_t x0 = jb.cx + (tx << tw_log), x1 = min(x0 + tw, jb.cx + jb.cw);
    const AxisTable *vt = reinterpret_cast<const AxisTable *>(arena + jb.vtab);
    const AxisTable *ht = reinterpret_cast<const AxisTable *>(arena + jb.htab);
    // the windows of an axis table move right monotonically: the column's window is [left of its first column, right end of its last)
    const uint32_t c0 = arena[ht->left_off + x0];
    const uint32_t ncols = arena[ht->left_off + x1 - 1u] + arena[ht->count_off + x1 - 1u] - c0;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const size_t pitch = (size_t)jb.sw * CS;
    // the horizontal weights of the columns lie back to back in the table: staged in LDS behind the f32 tile, coalesced
    // (read by output column in the horizontal pass they would be one cache line per lane)
    const uint32_t hw0 = arena[ht->woff_off + x0], hw1 = arena[ht->woff_off + x1 - 1u] + arena[ht->count_off + x1 - 1u];
    float *tile_w = tile_mid + kTileLdsFloats;
    float *tile_v = tile_w + kTileWeightFloats; // [source row of the band's window][output row of the band]: the vertical pass's weights
    const float *hweights = reinterpret_cast<const float *>(arena + ht->weights_off);
    for (uint32_t k = tid; k < hw1 - hw0; k += 256u) tile_w[k] = hweights[hw0 + k];
    // this thread's output column and the rows it takes in every tile (256 >> tw_log of them at a time)
    const uint32_t xx = tid & (tw - 1u), ysub = tid >> tw_log, ystep = 256u >> tw_log, ow = x1 - x0;
    const bool has_col = xx < ow;
    const uint32_t hx = x0 + min(xx, ow - 1u);
    const uint32_t hleft = arena[ht->left_off + hx], hn = arena[ht->count_off + hx];
    const float *hwp = tile_w + (arena[ht->woff_off + hx] - hw0);
    // vertical pass (all but the grayscale pre-op): the picture's band tables (fl_kernels.h TileVPlanHeader), and this thread's four bytes
    const TileVPlanHeader vp = *reinterpret_cast<const TileVPlanHeader *>(arena + jb.pad0);
    const uint32_t *vbands = arena + jb.pad0 + vp.bands_off;
    const float *vdense = reinterpret_cast<const float *>(arena + jb.pad0 + vp.dense_off);
    const uint32_t nbytes = ncols * (uint32_t)CS, b4 = tid * 4u;
    const uint32_t npitch = (ncols * (uint32_t)MC + 3u) & ~3u; // floats per row of the LDS tile: rows start 16-byte aligned, so a thread's four sums leave as one ds_write_b128
    const size_t col_off = (size_t)c0 * CS + b4;
    uint32_t inv = 0u; // Invert (color.rs Invert: 255 - c on the colour channels, alpha untouched) as an XOR mask of the four bytes
    if (PRE == PRE_INVERT) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t chn = (uint32_t)((col_off + j) % (uint32_t)CS);
            if (!((CS == 2 || CS == 4) && chn == (uint32_t)CS - 1u)) inv |= 0xffu << (8u * j);
        }
    }
    // Vertical pass, input-stationary by BYTE columns: without a pre-op that mixes channels a byte column is filtered like any other, so
    // a thread owns four consecutive bytes of the window, walks down the source rows the band's eight output rows touch -- each dword
    // loaded ONCE per band, kTilePrefetch of them in flight -- and feeds every row into all eight sums.  The weights are wave-uniform: a
    // dense [source row][output row] table in LDS, zero where a row lies outside an output row's window.  fma(v, 0, acc) leaves acc as
    // it is and a sum starts at +0, so each output row still sees exactly its taps, in tap order: the bits of the row-by-row form (one
    // workgroup-wide round of eight dependent loads per output row and 256 bytes; that form waited for the L2 78 % of the time,
    // profiles/r03_generic_sweep.txt).  The first rows of a band and its weight table are requested before the horizontal pass of
    // the band before it, so that their latency is spent under that pass.
    uint32_t rv = 0;                  // source rows of the band in hand (<= kTileVRows: the host checked)
    size_t goff = 0;                  // its first row's byte offset for this thread
    bool whole = false;               // every dword of this thread's column lies inside the source (all but the window's last thread in the picture's last rows)
    const uint8_t *pl = jb.src;       // the next row to request; it stops at the window's last row (requests past it repeat that row, unused)
    uint32_t ring[kTilePrefetch];
    float tvn[(kTileVRows * kTileRows) / 256u];
#pragma unroll
    for (uint32_t k = 0; k < kTilePrefetch; ++k) ring[k] = 0u;
    auto begin_band = [&](uint32_t y0) __attribute__((always_inline)) {
        const uint32_t bt = (y0 - jb.cy) / kTileRows; // band of the picture (the host's table is per picture, not per workgroup)
        const uint32_t top = vbands[2u * bt];
        rv = vbands[2u * bt + 1u];
        const float *dsrc = vdense + (size_t)bt * vp.rv_stride * kTileRows;
#pragma unroll
        for (uint32_t q = 0; q < (kTileVRows * kTileRows) / 256u; ++q) tvn[q] = tid + 256u * q < rv * kTileRows ? dsrc[tid + 256u * q] : 0.0f;
        goff = (size_t)top * pitch + col_off;
        whole = b4 < nbytes && goff + (size_t)(rv - 1u) * pitch + 4u <= (size_t)jb.src_bytes;
        if (whole) {
            pl = jb.src + goff;
#pragma unroll
            for (uint32_t k = 0; k < kTilePrefetch; ++k) {
                ring[k] = *reinterpret_cast<const u32_unaligned *>(pl);
                if (k + 1u < rv) pl += pitch;
            }
        }
    };
    auto publish_weights = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t q = 0; q < (kTileVRows * kTileRows) / 256u; ++q) tile_v[tid + 256u * q] = tvn[q];
    };
    if (PRE != PRE_GRAY) {
        begin_band(yb0);
        publish_weights();
        __syncthreads();
    }
    for (uint32_t y0 = yb0; y0 < yb1; y0 += kTileRows) {
        const uint32_t y1 = min(y0 + kTileRows, yb1);
        if (PRE != PRE_GRAY) {
            if (b4 < nbytes) {
                float acc[kTileRows][4];
#pragma unroll
                for (uint32_t o = 0; o < kTileRows; ++o)
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) acc[o][j] = 0.0f;
                auto add_row = [&](uint32_t r, uint32_t d) __attribute__((always_inline)) {
                    const f32x4 wa = *reinterpret_cast<const f32x4 *>(tile_v + r * kTileRows), wb = *reinterpret_cast<const f32x4 *>(tile_v + r * kTileRows + 4u);
                    const float v0 = (float)(d & 255u), v1 = (float)((d >> 8) & 255u), v2 = (float)((d >> 16) & 255u), v3 = (float)(d >> 24);
                    const float wr[kTileRows] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
                    for (uint32_t o = 0; o < kTileRows; ++o) {
                        acc[o][0] = __builtin_fmaf(v0, wr[o], acc[o][0]);
                        acc[o][1] = __builtin_fmaf(v1, wr[o], acc[o][1]);
                        acc[o][2] = __builtin_fmaf(v2, wr[o], acc[o][2]);
                        acc[o][3] = __builtin_fmaf(v3, wr[o], acc[o][3]);
                    }
                };
                // (the choice between dwords and bytes is made once per band, outside the loops: a branch inside them puts every load in a
                // block of its own, and the compiler drains vmcnt at each join)
                if (whole) {
                    for (uint32_t rb = 0; rb < rv; rb += kTilePrefetch) {
#pragma unroll
                        for (uint32_t k = 0; k < kTilePrefetch; ++k) {
                            const uint32_t r = rb + k, d = ring[k] ^ inv;
                            if (rb + kTilePrefetch < rv) { // (wave-uniform: the last round requests nothing, the ring is free for the next band)
                                ring[k] = *reinterpret_cast<const u32_unaligned *>(pl);
                                if (r + kTilePrefetch + 1u < rv) pl += pitch;
                            }
                            if (r < rv) add_row(r, d);
                        }
                    }
                } else {
                    for (uint32_t r = 0; r < rv; ++r) {
                        const size_t a = goff + (size_t)r * pitch;
                        uint32_t d = 0u;
                        for (uint32_t j = 0; j < 4u && a + j < (size_t)jb.src_bytes; ++j) d |= (uint32_t)jb.src[a + j] << (8u * j);
                        add_row(r, d ^ inv);
                    }
                }
#pragma unroll
                for (uint32_t o = 0; o < kTileRows; ++o) // (the last thread's sums past the window land in the row's padding)
                    *reinterpret_cast<f32x4 *>(tile_mid + (size_t)o * npitch + b4) = f32x4{acc[o][0], acc[o][1], acc[o][2], acc[o][3]};
            }
            if (y0 + kTileRows < yb1) begin_band(y0 + kTileRows); // the next band's first rows and weights: requested now, used after the horizontal pass
        } else {
            for (uint32_t ry = wave; ry < y1 - y0; ry += 4u) {
                const uint32_t oy = y0 + ry;
                const uint32_t left = arena[vt->left_off + oy], n = arena[vt->count_off + oy];
                const float *w = reinterpret_cast<const float *>(arena + vt->weights_off + arena[vt->woff_off + oy]);
                for (uint32_t col = lane; col < ncols; col += 64u) {
                    float acc[MC];
#pragma unroll
                    for (int k = 0; k < MC; ++k) acc[k] = 0.0f;
                    const uint8_t *p = jb.src + ((size_t)left * jb.sw + c0 + col) * CS;
                    for (uint32_t i = 0; i < n; ++i) {
                        uint32_t s[CS];
#pragma unroll
                        for (int k = 0; k < CS; ++k) s[k] = p[k];
                        float v[MC > CS ? MC : CS];
                        preop_pixel<CS, PRE>(s, v);
                        const float wi = w[i];
#pragma unroll
                        for (int k = 0; k < MC; ++k) acc[k] = __builtin_fmaf(v[k], wi, acc[k]);
                        p += pitch;
                    }
                    float *o = tile_mid + (size_t)ry * npitch + (size_t)col * MC;
#pragma unroll
                    for (int k = 0; k < MC; ++k) o[k] = acc[k];
                }
            }
        }
        __syncthreads();
        if (PRE != PRE_GRAY && y0 + kTileRows < yb1) publish_weights(); // (nobody reads this band's table any more; the barrier at the band's end publishes the next one)
        // Horizontal pass: a thread owns one output column and NR = tw / 32 of the tile's rows (ysub, ysub + ystep, ...), and takes
        // them through the taps TOGETHER: the weight, the block boundary of the grouped order and the tap's address are per column,
        // not per pixel (one pixel at a time spent two thirds of its vector instructions on them).
        if (has_col) {
            auto hpass = [&](auto nr_tag) __attribute__((always_inline)) {
                constexpr uint32_t NR = decltype(nr_tag)::value;
                const float *p = tile_mid + (size_t)ysub * npitch + (size_t)(hleft - c0) * MC;
                const uint32_t rstep = ystep * npitch;
                float acc[NR][MC], part[NR][MC];
#pragma unroll
                for (uint32_t q = 0; q < NR; ++q)
#pragma unroll
                    for (int k = 0; k < MC; ++k) { acc[q][k] = 0.0f; part[q][k] = 0.0f; }
                for (uint32_t i = 0; i < hn; ++i) {
                    if (GROUPED && i != 0 && ((hleft + i) & 3u) == 0u) {
#pragma unroll
                        for (uint32_t q = 0; q < NR; ++q)
#pragma unroll
                            for (int k = 0; k < MC; ++k) { acc[q][k] = acc[q][k] + part[q][k]; part[q][k] = 0.0f; }
                    }
                    const float wi = hwp[i];
#pragma unroll
                    for (uint32_t q = 0; q < NR; ++q)
#pragma unroll
                        for (int k = 0; k < MC; ++k) part[q][k] = __builtin_fmaf(p[q * rstep + k], wi, part[q][k]);
                    p += MC;
                }
#pragma unroll
                for (uint32_t q = 0; q < NR; ++q) {
                    const uint32_t yy = ysub + q * ystep;
                    if (yy >= y1 - y0) break; // (rows past a short last tile were computed on whatever the LDS held: never stored)
                    uint32_t cc[MC];
#pragma unroll
                    for (int k = 0; k < MC; ++k) cc[k] = round_u8(acc[q][k] + part[q][k]);
                    store_pixel<MC, LB>(jb.dst, (jb.oy + (y0 - jb.cy) + yy) * jb.dw + jb.ox + (x0 - jb.cx) + xx, cc, jb.fill);
                }
            };
            if (tw_log >= 8u) hpass(std::integral_constant<uint32_t, 8>{});
            else if (tw_log == 7u) hpass(std::integral_constant<uint32_t, 4>{});
            else if (tw_log == 6u) hpass(std::integral_constant<uint32_t, 2>{});
            else if (ysub < kTileRows) hpass(std::integral_constant<uint32_t, 1>{});
        }
        __syncthreads(); // the next tile's vertical pass overwrites the LDS tile
    }
}

// launch wrappers (called from the host runtime; all asynchronous on `st`)

hipError_t launch_vpass_generic(const LaunchGeneric &g, hipStream_t st)
{
    dim3 grid((g.max_sw * g.max_rh + 255u) / 256u, g.njobs);
    return dispatch_cs_pre(g.cs, g.pre, [&](auto cs, auto pre) {
        hipLaunchKernelGGL((vpass_generic_kernel<decltype(cs)::value, decltype(pre)::value>), grid, dim3(256), 0, st, g.jobs, g.arena, g.mid, g.job_base);
        return hipGetLastError();
    });
}

hipError_t launch_hpass_generic(const LaunchGeneric &g, hipStream_t st)
{
    dim3 grid((g.max_cw * g.max_ch + 255u) / 256u, g.njobs);
    auto launch = [&](auto mc) {
        return dispatch_bool(g.letterbox, [&](auto lb) { return dispatch_bool(g.grouped, [&](auto grouped) {
            hipLaunchKernelGGL((hpass_generic_kernel<decltype(mc)::value, decltype(lb)::value, decltype(grouped)::value>), grid, dim3(256), 0, st, g.jobs, g.arena, g.mid, g.job_base);
            return hipGetLastError();
        }); });
    };
    switch (mid_channels(g.cs, g.pre)) {
    case 1: return launch(std::integral_constant<int, 1>{});
    case 2: return launch(std::integral_constant<int, 2>{});
    case 3: return launch(std::integral_constant<int, 3>{});
    case 4: return launch(std::integral_constant<int, 4>{});
    }
    return hipErrorInvalidValue;
}

hipError_t launch_tile_resample(const LaunchGeneric &g, hipStream_t st)
{
    // grid.x: (tile columns of the widest kept window at the narrowest tile width) x bands of rows -- enough bands that the chip sees
    // a few thousand workgroups also when the batch is one picture
    const uint32_t cols = (g.max_cw + g.tile_w_min - 1u) / g.tile_w_min;
    const uint32_t max_bands = (g.max_ch + kTileRows - 1u) / kTileRows;
    const uint32_t nbands = std::max(1u, std::min(max_bands, (4096u + cols * g.njobs - 1u) / (cols * g.njobs)));
    dim3 grid(cols * nbands, g.njobs);
    const size_t lds = (size_t)(kTileLdsFloats + kTileWeightFloats + kTileVRows * kTileRows) * sizeof(float);
    return dispatch_cs_pre(g.cs, g.pre, [&](auto cs, auto pre) {
        return dispatch_bool(g.letterbox, [&](auto lb) { return dispatch_bool(g.grouped, [&](auto grouped) {
            const auto k = resample_tile_kernel<decltype(cs)::value, decltype(pre)::value, decltype(lb)::value, decltype(grouped)::value>;
            static std::atomic<uint64_t> attr_set{0}; // one per kernel (the lambda is instantiated per kernel): the attribute is per function and device
            if (hipError_t e = set_max_lds_once(attr_set, (int)lds, {reinterpret_cast<const void *>(k)}); e != hipSuccess) return e;
            hipLaunchKernelGGL(k, grid, dim3(256), lds, st, g.jobs, g.arena, g.job_base, nbands);
            return hipGetLastError();
        }); });
    });
}

} // namespace fl
