// fl_place.hip -- kernels that move pixels without filtering them.
//   place_kernel / place4_kernel   pointwise placement: requests that only grayscale, invert, crop or letterbox (S1_PLACE), the
//                                  Nearest gather of animated-GIF frames (S1_NEAREST), and the border fill enqueue_launches puts
//                                  in front of the letterboxed S1_TILE / S1_WTILE / S1_GENERIC resamples.
//   orient_kernel                  EXIF orientation pre-pass, the first launches of enqueue_launches.
#include "fl_kernel_common.h"
#include "fl_kernels.h"

namespace fl {

// ---------------------------------------------------------------------------
// Pointwise placement: no resampling.  dst(x,y) = preop(src(x-ox+cx, y-oy+cy))
// converted to the destination layout, or the fill colour outside the placed
// window.  Covers grayscale/invert-only requests, letterbox-only requests and
// the border fill of resampled letterboxed images (BORDER_ONLY).
// ---------------------------------------------------------------------------

// FilterType::Nearest through image 0.25.6 sample.rs (support 0.0, box kernel): one tap of weight 1 at
// clamp(floor((o + 0.5) * ratio), 0, in - 1), ratio = in as f32 / out as f32 computed on the host
// (animated-GIF frames, reference handler.rs:336-341).
__device__ __forceinline__ uint32_t nearest_tap(uint32_t o, uint32_t ratio_bits, uint32_t in_size)
{
    const float c = ((float)o + 0.5f) * __uint_as_float(ratio_bits);
    const int left = (int)floorf(c);
    return (uint32_t)min(max(left, 0), (int)in_size - 1);
}

template <int CS, int PRE, bool LB, bool BORDER_ONLY, bool NEAREST = false>
__global__ __launch_bounds__(256) void place_kernel(const Job *__restrict__ jobs, uint32_t job_base)
{
    constexpr int MC = mid_channels(CS, PRE);
    const Job jb = jobs[job_base + blockIdx.y];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;  // flat over the destination of this job
    if (idx >= jb.dh * jb.dw) return;
    const uint32_t y = idx / jb.dw, x = idx - y * jb.dw;
    const bool inside = x >= jb.ox && x < jb.ox + jb.cw && y >= jb.oy && y < jb.oy + jb.ch;
    if (!inside) {
        if (LB) reinterpret_cast<uint32_t *>(jb.dst)[y * jb.dw + x] = jb.fill;
        return;
    }
    if (BORDER_ONLY) return;
    uint32_t sy = y - jb.oy + jb.cy, sx = x - jb.ox + jb.cx;
    if (NEAREST) { sy = nearest_tap(sy, jb.vtab, jb.sh); sx = nearest_tap(sx, jb.htab, jb.sw); }
    const uint8_t *p = jb.src + ((size_t)sy * jb.sw + sx) * CS;
    uint32_t s[CS];
#pragma unroll
    for (int k = 0; k < CS; ++k) s[k] = p[k];
    float v[MC > CS ? MC : CS];
    preop_pixel<CS, PRE>(s, v);
    uint32_t c[MC];
#pragma unroll
    for (int k = 0; k < MC; ++k) c[k] = (uint32_t)v[k];
    store_pixel<MC, LB>(jb.dst, y * jb.dw + x, c, jb.fill);
}

// The same placement, four destination pixels of a row per thread: one thread per pixel with byte loads and stores ran a
// grayscale-only 1080p request at 0.2 of the HBM peak (tools/experiments/generic_sweep.py).  Where the four pixels lie inside the
// picture's window the source bytes come as CS dwords (gfx950 loads a dword from any byte address) and the result leaves as
// dwords; threads that straddle the window's edge fall back to the pixel-wise path above.  No arithmetic differs.
typedef uint32_t __attribute__((aligned(1))) u32_any; // a dword at any byte address
template <int CS, int PRE, bool LB>
__global__ __launch_bounds__(256) void place4_kernel(const Job *__restrict__ jobs, uint32_t job_base)
{
    constexpr int MC = mid_channels(CS, PRE);
    const Job jb = jobs[job_base + blockIdx.z];
    const uint32_t y = blockIdx.y, x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (y >= jb.dh || x0 >= jb.dw) return;
    const bool row_in = y >= jb.oy && y < jb.oy + jb.ch;
    if (row_in && x0 >= jb.ox && x0 + 4u <= jb.ox + jb.cw) {
        const uint32_t sy = y - jb.oy + jb.cy, sx = x0 - jb.ox + jb.cx;
        const uint8_t *p = jb.src + ((size_t)sy * jb.sw + sx) * CS;
        uint32_t d[CS];
#pragma unroll
        for (int j = 0; j < CS; ++j) d[j] = *reinterpret_cast<const u32_any *>(p + 4 * j);
        uint32_t c[4][MC];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            uint32_t s4[CS];
#pragma unroll
            for (int k = 0; k < CS; ++k) { const int b = px * CS + k; s4[k] = (d[b >> 2] >> (8 * (b & 3))) & 255u; }
            float v[MC > CS ? MC : CS];
            preop_pixel<CS, PRE>(s4, v);
#pragma unroll
            for (int k = 0; k < MC; ++k) c[px][k] = (uint32_t)v[k];
        }
        if (LB) {
#pragma unroll
            for (int px = 0; px < 4; ++px) store_pixel<MC, true>(jb.dst, y * jb.dw + x0 + px, c[px], jb.fill);
        } else {
            uint8_t *o = jb.dst + ((size_t)y * jb.dw + x0) * MC;
#pragma unroll
            for (int j = 0; j < MC; ++j) {
                uint32_t w = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) { const int b = 4 * j + q; w |= c[b / MC][b % MC] << (8 * q); }
                *reinterpret_cast<u32_any *>(o + 4 * j) = w;
            }
        }
        return;
    }
    for (uint32_t x = x0; x < min(x0 + 4u, jb.dw); ++x) {
        const bool inside = row_in && x >= jb.ox && x < jb.ox + jb.cw;
        if (!inside) {
            if (LB) reinterpret_cast<uint32_t *>(jb.dst)[y * jb.dw + x] = jb.fill;
            continue;
        }
        const uint8_t *p = jb.src + ((size_t)(y - jb.oy + jb.cy) * jb.sw + (x - jb.ox + jb.cx)) * CS;
        uint32_t s1[CS];
#pragma unroll
        for (int k = 0; k < CS; ++k) s1[k] = p[k];
        float v[MC > CS ? MC : CS];
        preop_pixel<CS, PRE>(s1, v);
        uint32_t c1[MC];
#pragma unroll
        for (int k = 0; k < MC; ++k) c1[k] = (uint32_t)v[k];
        store_pixel<MC, LB>(jb.dst, y * jb.dw + x, c1, jb.fill);
    }
}

// ---------------------------------------------------------------------------
// EXIF orientation (DynamicImage::apply_orientation, image 0.25.6 metadata::Orientation + imageops::rotate90 /
// rotate180 / rotate270 / flip_horizontal / flip_vertical): a pure pixel permutation, one thread per
// destination pixel.  jb.sw x jb.sh = SOURCE size, jb.dw x jb.dh = oriented size, jb.fill = EXIF code 2..8.
// ---------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void orient_kernel(const Job *__restrict__ jobs, uint32_t job_base)
{
    const Job jb = jobs[job_base + blockIdx.z];
    const uint32_t y = blockIdx.y, x = blockIdx.x * 256u + threadIdx.x;
    if (y >= jb.dh || x >= jb.dw) return;
    const uint32_t W = jb.sw, H = jb.sh;
    uint32_t sx, sy;
    switch (jb.fill) {
    case 2: sx = W - 1u - x; sy = y; break;              // FlipHorizontal
    case 3: sx = W - 1u - x; sy = H - 1u - y; break;     // Rotate180
    case 4: sx = x; sy = H - 1u - y; break;              // FlipVertical
    case 5: sx = y; sy = x; break;                       // Rotate90FlipH (transpose)
    case 6: sx = y; sy = H - 1u - x; break;              // Rotate90
    case 7: sx = W - 1u - y; sy = H - 1u - x; break;     // Rotate270FlipH (transverse)
    case 8: sx = W - 1u - y; sy = x; break;              // Rotate270
    default: sx = x; sy = y; break;
    }
    const uint8_t *p = jb.src + ((size_t)sy * W + sx) * C;
    uint8_t *o = jb.dst + ((size_t)y * jb.dw + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = p[c];
}

template <int CS, int PRE, bool LB>
static hipError_t launch_place_t(const LaunchGeneric &g, bool border_only, hipStream_t st)
{
    dim3 grid((g.max_dw * g.max_dh + 255u) / 256u, g.njobs);
    if (g.nearest) hipLaunchKernelGGL((place_kernel<CS, PRE, LB, false, true>), grid, dim3(256), 0, st, g.jobs, g.job_base);
    else if (border_only) {
        if constexpr (!LB) return hipSuccess;
        else { hipLaunchKernelGGL((place_kernel<CS, PRE, true, true>), grid, dim3(256), 0, st, g.jobs, g.job_base); }
    } else if (g.max_dh <= 65535u && g.njobs <= 65535u && !g.no_place4) { // (grid limits of the y and z dimensions)
        dim3 grid4(((g.max_dw + 3u) / 4u + 255u) / 256u, g.max_dh, g.njobs);
        hipLaunchKernelGGL((place4_kernel<CS, PRE, LB>), grid4, dim3(256), 0, st, g.jobs, g.job_base);
    } else hipLaunchKernelGGL((place_kernel<CS, PRE, LB, false>), grid, dim3(256), 0, st, g.jobs, g.job_base);
    return hipGetLastError();
}

hipError_t launch_place(const LaunchGeneric &g, bool border_only, hipStream_t st)
{
    return dispatch_cs_pre(g.cs, g.pre, [&](auto cs, auto pre) {
        return dispatch_bool(g.letterbox, [&](auto lb) { return launch_place_t<decltype(cs)::value, decltype(pre)::value, decltype(lb)::value>(g, border_only, st); });
    });
}

hipError_t launch_orient(const LaunchGeneric &g, hipStream_t st)
{
    dim3 grid((g.max_dw + 255u) / 256u, g.max_dh, g.njobs);
    switch (g.cs) {
    case 1: hipLaunchKernelGGL(orient_kernel<1>, grid, dim3(256), 0, st, g.jobs, g.job_base); break;
    case 2: hipLaunchKernelGGL(orient_kernel<2>, grid, dim3(256), 0, st, g.jobs, g.job_base); break;
    case 3: hipLaunchKernelGGL(orient_kernel<3>, grid, dim3(256), 0, st, g.jobs, g.job_base); break;
    case 4: hipLaunchKernelGGL(orient_kernel<4>, grid, dim3(256), 0, st, g.jobs, g.job_base); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace fl
