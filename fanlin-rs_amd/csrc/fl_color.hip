// fl_color.hip -- colour conversions around the resample: no filtering, integer or f32 arithmetic in the reference's order.
//   jfif444* / webp420*    planar front ends of the host encoders (FLGPU_FE_JFIF444 / FLGPU_FE_WEBP420), the fe_launches of
//                          enqueue_launches (fl_batch.cpp).
//   ycck_to_cmyk_kernel,   CMYK / YCCK JPEG sources on their way to RGB, launched by the CMYK context (fl_cmyk_ctx.cpp) before
//   cmyk_clut_kernel       the batch proper.
#include "fl_kernels.h"
#include "fl_pixel.h"

namespace fl {

// ---------------------------------------------------------------------------
// Encoder colour front ends
// ---------------------------------------------------------------------------

// DynamicImage get_pixel -> Rgba<u8>: Luma -> (l,l,l,255), LumaA -> (l,l,l,a), Rgb -> (r,g,b,255)
// image 0.25.6 codecs/jpeg/encoder.rs rgb_to_ycbcr (f32, truncating) on 8x8-padded planes
// (copy_blocks_ycbcr / pixel_at_or_near replicate the last column and row).
__global__ __launch_bounds__(256) void jfif444_kernel(const FrontendJob *__restrict__ fjobs, uint32_t job_base)
{
    const FrontendJob fj = fjobs[job_base + blockIdx.z];
    const uint32_t y = blockIdx.y;
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (y >= fj.plane_h || x >= fj.plane_w) return;
    const uint32_t sx = x < fj.w ? x : fj.w - 1u, sy = y < fj.h ? y : fj.h - 1u;
    uint32_t ri, gi, bi, ai;
    load_rgba(fj.src + ((size_t)sy * fj.w + sx) * fj.c, fj.c, ri, gi, bi, ai);
    const float max = 255.0f;
    const float r = (float)ri, g = (float)gi, b = (float)bi;
    const float yy = 76.245f / max * r + 149.685f / max * g + 29.07f / max * b;
    const float cb = -43.0185f / max * r - 84.4815f / max * g + 127.5f / max * b + 128.0f;
    const float cr = 127.5f / max * r - 106.7685f / max * g - 20.7315f / max * b + 128.0f;
    const size_t plane = (size_t)fj.plane_w * fj.plane_h, o = (size_t)y * fj.plane_w + x;
    fj.dst[o] = sat_u8(yy);
    fj.dst[plane + o] = sat_u8(cb);
    fj.dst[2 * plane + o] = sat_u8(cr);
}

// libwebp dsp/yuv.h fixed point (YUV_FIX = 16) + picture_csp_enc.c gamma-corrected 2x2 chroma averaging.
__device__ __forceinline__ int webp_clip_uv(int uv, int rounding)
{
    uv = (uv + rounding + (128 << 18)) >> 18;
    return ((uv & ~0xff) == 0) ? uv : (uv < 0) ? 0 : 255;
}
__device__ __forceinline__ int webp_linear_to_gamma(const int32_t *lin2gam, uint32_t base_value, int shift)
{
    const int v = (int)(base_value << shift);
    const int tab_pos = v >> 9;              // GAMMA_TAB_FIX + 2
    const int x = v & 511;                   // (kGammaTabScale << 2) - 1
    const int y = lin2gam[tab_pos + 1] * x + lin2gam[tab_pos] * (512 - x);
    return (y + 64) >> 7;                    // kGammaTabRounder, GAMMA_TAB_FIX
}

// One 2x2 block of libwebp's chroma down-sampling (picture_csp_enc.c AccumulateRGB / AccumulateRGBA): the four pixels
// (edge blocks repeat the last column / row: libwebp's SUM2 with shift 1, or step = 0 / rgb_stride = 0, are the same
// numbers) are averaged in linear light; a block that is neither fully opaque nor fully transparent weights them by
// alpha: LinearToGammaWeighted = LinearToGamma((sum a_i * GammaToLinear(c_i) * kInvAlpha[a]) >> 17), kInvAlpha[a] = 2^19 / a.
struct WebpBlock {
    uint32_t sr = 0, sg = 0, sb = 0;     // plain sums of GammaToLinear
    uint32_t wr = 0, wg = 0, wb = 0;     // alpha-weighted sums
    uint32_t a = 0;
    bool translucent = false;
    __device__ __forceinline__ void add(const int32_t *gam2lin, uint32_t r, uint32_t g, uint32_t b, uint32_t alpha)
    {
        const uint32_t lr = (uint32_t)gam2lin[r], lg = (uint32_t)gam2lin[g], lb = (uint32_t)gam2lin[b];
        sr += lr; sg += lg; sb += lb;
        wr += alpha * lr; wg += alpha * lg; wb += alpha * lb;
        a += alpha;
        translucent |= alpha != 255u;
    }
    __device__ __forceinline__ void finish(const int32_t *lin2gam, int &r, int &g, int &b) const
    {
        if (a == 4u * 255u || a == 0u) {
            r = webp_linear_to_gamma(lin2gam, sr, 0);
            g = webp_linear_to_gamma(lin2gam, sg, 0);
            b = webp_linear_to_gamma(lin2gam, sb, 0);
        } else {
            const uint32_t inv = (1u << 19) / a; // rare path: a real division is fine
            r = webp_linear_to_gamma(lin2gam, (wr * inv) >> 17, 0);
            g = webp_linear_to_gamma(lin2gam, (wg * inv) >> 17, 0);
            b = webp_linear_to_gamma(lin2gam, (wb * inv) >> 17, 0);
        }
    }
};

__global__ __launch_bounds__(256) void webp420_kernel(const FrontendJob *__restrict__ fjobs, const uint32_t *__restrict__ arena,
                                                      uint32_t gamma_off, uint32_t job_base)
{
    const FrontendJob fj = fjobs[job_base + blockIdx.z];
    const uint32_t by = blockIdx.y;
    const uint32_t bx = blockIdx.x * 256u + threadIdx.x;
    if (by >= fj.chroma_h || bx >= fj.chroma_w) return;
    const int32_t *gam2lin = reinterpret_cast<const int32_t *>(arena + gamma_off);       // [256]
    const int32_t *lin2gam = gam2lin + 256;                                               // [33]
    const uint32_t w = fj.w, h = fj.h, c = fj.c;
    const uint32_t x0 = 2u * bx, y0 = 2u * by;
    const uint32_t x1 = x0 + 1u < w ? x0 + 1u : x0;     // odd width: SUM2 path
    const uint32_t y1 = y0 + 1u < h ? y0 + 1u : y0;     // odd height: rgb_stride = 0
    uint8_t *Y = fj.dst, *U = fj.dst + (size_t)w * h, *V = U + (size_t)fj.chroma_w * fj.chroma_h, *A = V + (size_t)fj.chroma_w * fj.chroma_h;
    WebpBlock blk;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t px = (k & 1) ? x1 : x0, py = (k & 2) ? y1 : y0;
        uint32_t r, g, b, a;
        load_rgba(fj.src + ((size_t)py * w + px) * c, c, r, g, b, a);
        // luma and alpha of each real pixel (duplicates of the edge replicate are rewritten with the same value)
        const int luma = 16839 * (int)r + 33059 * (int)g + 6420 * (int)b;
        Y[(size_t)py * w + px] = (uint8_t)((luma + (1 << 15) + (16 << 16)) >> 16);
        A[(size_t)py * w + px] = (uint8_t)a;
        blk.add(gam2lin, r, g, b, a);
    }
    int r, g, b;
    blk.finish(lin2gam, r, g, b);
    U[(size_t)by * fj.chroma_w + bx] = (uint8_t)webp_clip_uv(-9719 * r - 19081 * g + 28800 * b, 1 << 17);
    V[(size_t)by * fj.chroma_w + bx] = (uint8_t)webp_clip_uv(+28800 * r - 24116 * g - 4684 * b, 1 << 17);
    if (blk.translucent && fj.status) atomicOr(fj.status, 1u);
}

// Rgba8 fast paths of the front ends (every letterboxed output is Rgba8): 4 pixels per thread, dword loads,
// dword stores per plane.  Same arithmetic as the generic kernels above.
__global__ __launch_bounds__(256) void jfif444_rgba_kernel(const FrontendJob *__restrict__ fjobs, uint32_t job_base)
{
    const FrontendJob fj = fjobs[job_base + blockIdx.y];
    const uint32_t q = fj.plane_w >> 2;                        // 4-pixel groups per plane row (plane_w is a multiple of 8)
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;      // flat over rows x groups: narrow planes still fill the waves
    if (idx >= q * fj.plane_h) return;
    const uint32_t y = idx / q, x = (idx - y * q) * 4u;
    const uint32_t sy = y < fj.h ? y : fj.h - 1u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(fj.src), 0, (int)(fj.w * fj.h * 4u), 0x00020000);
    uint32_t yy = 0, cb = 0, cr = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t sx = x + k < fj.w ? x + k : fj.w - 1u; // replicate the last column into the padding
        const uint32_t d = __builtin_amdgcn_raw_buffer_load_b32(rs, (sy * fj.w + sx) * 4u, 0, 0);
        uint32_t a, b, c;
        jfif_px(d, a, b, c);
        yy |= a << (8 * k); cb |= b << (8 * k); cr |= c << (8 * k);
    }
    const size_t plane = (size_t)fj.plane_w * fj.plane_h, o = (size_t)y * fj.plane_w + x;
    uint8_t *dst = fj.dst;
    *reinterpret_cast<uint32_t *>(dst + o) = yy;
    *reinterpret_cast<uint32_t *>(dst + plane + o) = cb;
    *reinterpret_cast<uint32_t *>(dst + 2 * plane + o) = cr;
}

__global__ __launch_bounds__(256) void webp420_rgba_kernel(const FrontendJob *__restrict__ fjobs, const uint32_t *__restrict__ arena,
                                                           uint32_t gamma_off, uint32_t job_base)
{
    const FrontendJob fj = fjobs[job_base + blockIdx.y];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x; // flat over chroma samples
    if (idx >= fj.chroma_w * fj.chroma_h) return;
    const uint32_t by = idx / fj.chroma_w, bx = idx - by * fj.chroma_w;
    const int32_t *gam2lin = reinterpret_cast<const int32_t *>(arena + gamma_off);
    const int32_t *lin2gam = gam2lin + 256;
    const uint32_t w = fj.w, h = fj.h;
    const uint32_t x0 = 2u * bx, y0 = 2u * by;
    const uint32_t x1 = x0 + 1u < w ? x0 + 1u : x0;
    const uint32_t y1 = y0 + 1u < h ? y0 + 1u : y0;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(fj.src), 0, (int)(w * h * 4u), 0x00020000);
    uint8_t *Y = fj.dst, *U = fj.dst + (size_t)w * h, *V = U + (size_t)fj.chroma_w * fj.chroma_h, *A = V + (size_t)fj.chroma_w * fj.chroma_h;
    WebpBlock blk;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t px = (k & 1) ? x1 : x0, py = (k & 2) ? y1 : y0;
        const uint32_t d = __builtin_amdgcn_raw_buffer_load_b32(rs, (py * w + px) * 4u, 0, 0);
        const uint32_t r = d & 255u, g = (d >> 8) & 255u, b = (d >> 16) & 255u, a = d >> 24;
        const int luma = 16839 * (int)r + 33059 * (int)g + 6420 * (int)b;
        Y[(size_t)py * w + px] = (uint8_t)((luma + (1 << 15) + (16 << 16)) >> 16);
        A[(size_t)py * w + px] = (uint8_t)a;
        blk.add(gam2lin, r, g, b, a);
    }
    int r, g, b;
    blk.finish(lin2gam, r, g, b);
    U[(size_t)by * fj.chroma_w + bx] = (uint8_t)webp_clip_uv(-9719 * r - 19081 * g + 28800 * b, 1 << 17);
    V[(size_t)by * fj.chroma_w + bx] = (uint8_t)webp_clip_uv(+28800 * r - 24116 * g - 4684 * b, 1 << 17);
    if (blk.translucent && fj.status) atomicOr(fj.status, 1u);
}

// reference src/handler.rs:423-438: per pixel (Y, Cb, Cr, K) -> (clamp(R), clamp(G), clamp(B), 255 - K), f32 with
// truncating casts, evaluated in the reference's operation order (this file is built with -ffp-contract=off)
__device__ __forceinline__ uint32_t ycck_pixel(uint32_t d)
{
    const float y = (float)(d & 255u), cb = (float)((d >> 8) & 255u), cr = (float)((d >> 16) & 255u);
    float r = y + 1.40200f * cr - 179.456f;
    float g = y - 0.34414f * cb - 0.71414f * cr + 135.45984f;
    float b = y + 1.77200f * cb - 226.816f;
    r = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
    g = g < 0.0f ? 0.0f : (g > 255.0f ? 255.0f : g);
    b = b < 0.0f ? 0.0f : (b > 255.0f ? 255.0f : b);
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | ((255u - (d >> 24)) << 24);
}

__global__ __launch_bounds__(256) void ycck_to_cmyk_kernel(uint32_t *__restrict__ px, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    px[i] = ycck_pixel(px[i]);
}

// ---------------------------------------------------------------------------
// CMYK_8 -> RGB_8 through a baked device-link CLUT: what lcms2's transform_pixels does for the transform the
// reference builds (src/handler.rs:469-493: CMYK profile -> sRGB, Perceptual, NO_CACHE).  Little CMS 2 optimises
// that transform into ONE 17^4 x 3 u16 table (cmsopt.c OptimizeByResampling) and evaluates every pixel with
// cmsintrp.c Eval4Inputs: tetrahedral interpolation over inputs 1..3 on the two table slices that bracket
// input 0, then a linear blend, all in 16.16 fixed point with 32-bit wrap-around.  This kernel is that
// arithmetic (formatters Unroll4Bytes / Pack3Bytes included); the table is baked on the host
// (fl_cmyk.cpp).  Table nodes are padded to 4 x u16 so that a node is one 8-byte load.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int32_t lcms_to_fixed_domain(int32_t a)
{
    return (int32_t)((uint32_t)a + (uint32_t)((int32_t)((uint32_t)a + 0x7fffu) / 0xffff));
}

struct ClutNode { int32_t c[3]; };
__device__ __forceinline__ ClutNode clut_load(const uint2 *__restrict__ t, uint32_t idx)
{
    const uint2 v = t[idx];
    return ClutNode{{(int32_t)(v.x & 0xffffu), (int32_t)(v.x >> 16), (int32_t)(v.y & 0xffffu)}};
}

// tetrahedral interpolation inside slice `base`: the six cases of Eval4Inputs collapse to "walk the cube
// from (0,0,0) to (1,1,1) along the axes in descending order of their fractions" (ties give equal sums)
__device__ __forceinline__ void clut_tetra(const uint2 *__restrict__ t, uint32_t base, uint32_t X0, uint32_t X1, uint32_t Y0,
                                           uint32_t Y1, uint32_t Z0, uint32_t Z1, int32_t rx, int32_t ry, int32_t rz, uint32_t out[3])
{
    uint32_t a1, a2; // the two intermediate vertices
    int32_t r1, r2, r3;
    if (rx >= ry && ry >= rz)      { a1 = X1 + Y0 + Z0; a2 = X1 + Y1 + Z0; r1 = rx; r2 = ry; r3 = rz; }
    else if (rx >= rz && rz >= ry) { a1 = X1 + Y0 + Z0; a2 = X1 + Y0 + Z1; r1 = rx; r2 = rz; r3 = ry; }
    else if (rz >= rx && rx >= ry) { a1 = X0 + Y0 + Z1; a2 = X1 + Y0 + Z1; r1 = rz; r2 = rx; r3 = ry; }
    else if (ry >= rx && rx >= rz) { a1 = X0 + Y1 + Z0; a2 = X1 + Y1 + Z0; r1 = ry; r2 = rx; r3 = rz; }
    else if (ry >= rz && rz >= rx) { a1 = X0 + Y1 + Z0; a2 = X0 + Y1 + Z1; r1 = ry; r2 = rz; r3 = rx; }
    else                           { a1 = X0 + Y0 + Z1; a2 = X0 + Y1 + Z1; r1 = rz; r2 = ry; r3 = rx; }
    const ClutNode v0 = clut_load(t, base + X0 + Y0 + Z0), v1 = clut_load(t, base + a1), v2 = clut_load(t, base + a2),
                   v3 = clut_load(t, base + X1 + Y1 + Z1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t rest = (uint32_t)(v1.c[k] - v0.c[k]) * (uint32_t)r1 + (uint32_t)(v2.c[k] - v1.c[k]) * (uint32_t)r2 +
                              (uint32_t)(v3.c[k] - v2.c[k]) * (uint32_t)r3;
        const int32_t f = lcms_to_fixed_domain((int32_t)rest);
        out[k] = (uint32_t)(v0.c[k] + (((int32_t)((uint32_t)f + 0x8000u)) >> 16)) & 0xffffu;
    }
}

__device__ __forceinline__ uint32_t cmyk_clut_pixel(const uint2 *__restrict__ t, uint32_t grid, uint32_t d)
{
    const uint32_t domain = grid - 1u;
    const uint32_t sz = 1u, sy = grid, sx = grid * grid, sk = grid * grid * grid; // node strides of inputs 3, 2, 1, 0
    uint32_t i0[4], step[4];
    int32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = (d >> (8 * k)) & 255u;
        const uint32_t in16 = b * 257u;                                  // FROM_8_TO_16
        const int32_t f = lcms_to_fixed_domain((int32_t)(in16 * domain));
        i0[k] = (uint32_t)f >> 16;
        r[k] = f & 0xffff;
        step[k] = b == 255u ? 0u : 1u;                                   // Input == 0xFFFF: no upper neighbour
    }
    const uint32_t K0 = sk * i0[0], K1 = K0 + sk * step[0];
    const uint32_t X0 = sx * i0[1], X1 = X0 + sx * step[1];
    const uint32_t Y0 = sy * i0[2], Y1 = Y0 + sy * step[2];
    const uint32_t Z0 = sz * i0[3], Z1 = Z0 + sz * step[3];
    uint32_t t1[3], t2[3];
    clut_tetra(t, K0, X0, X1, Y0, Y1, Z0, Z1, r[1], r[2], r[3], t1);
    clut_tetra(t, K1, X0, X1, Y0, Y1, Z0, Z1, r[1], r[2], r[3], t2);
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t dif = (t2[k] - t1[k]) * (uint32_t)r[0] + 0x8000u;      // LinearInterp
        dif = ((dif >> 16) + t1[k]) & 0xffffu;
        o |= ((dif * 65281u + 8388608u) >> 24) << (8 * k);              // FROM_16_TO_8
    }
    return o;
}

// 4 pixels per thread: one 16-byte load, three dword stores.  n4 = ceil(n / 4); the buffers are padded to that.
template <bool YCCK>
__global__ __launch_bounds__(256) void cmyk_clut_kernel(const uint4 *__restrict__ src, uint32_t *__restrict__ dst,
                                                        const uint2 *__restrict__ clut, uint32_t grid, uint64_t n4)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n4) return;
    const uint4 q = src[i];
    uint32_t p[4] = {q.x, q.y, q.z, q.w}, o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (YCCK) p[k] = ycck_pixel(p[k]);
        o[k] = cmyk_clut_pixel(clut, grid, p[k]);
    }
    dst[i * 3 + 0] = o[0] | (o[1] << 24);
    dst[i * 3 + 1] = (o[1] >> 8) | (o[2] << 16);
    dst[i * 3 + 2] = (o[2] >> 16) | (o[3] << 8);
}

hipError_t launch_cmyk_clut(const void *src, void *dst, const void *clut, uint32_t grid, uint64_t n_pixels, bool ycck, hipStream_t st)
{
    const uint64_t n4 = (n_pixels + 3) / 4;
    if (n4 == 0) return hipSuccess;
    const dim3 g((unsigned)((n4 + 255) / 256));
    if (ycck) hipLaunchKernelGGL(cmyk_clut_kernel<true>, g, dim3(256), 0, st, static_cast<const uint4 *>(src), static_cast<uint32_t *>(dst),
                                 static_cast<const uint2 *>(clut), grid, n4);
    else hipLaunchKernelGGL(cmyk_clut_kernel<false>, g, dim3(256), 0, st, static_cast<const uint4 *>(src), static_cast<uint32_t *>(dst),
                            static_cast<const uint2 *>(clut), grid, n4);
    return hipGetLastError();
}

hipError_t launch_ycck_to_cmyk(uint32_t *px, uint64_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ycck_to_cmyk_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, px, n);
    return hipGetLastError();
}

hipError_t launch_jfif444(const FrontendJob *fjobs, uint32_t job_base, uint32_t njobs, uint32_t max_pw, uint32_t max_ph,
                          bool all_rgba_aligned, hipStream_t st)
{
    if (all_rgba_aligned) {
        dim3 grid4(((max_pw / 4u) * max_ph + 255u) / 256u, njobs);
        hipLaunchKernelGGL(jfif444_rgba_kernel, grid4, dim3(256), 0, st, fjobs, job_base);
        return hipGetLastError();
    }
    dim3 grid((max_pw + 255u) / 256u, max_ph, njobs);
    hipLaunchKernelGGL(jfif444_kernel, grid, dim3(256), 0, st, fjobs, job_base);
    return hipGetLastError();
}

hipError_t launch_webp420(const FrontendJob *fjobs, const uint32_t *arena, uint32_t gamma_off, uint32_t job_base,
                          uint32_t njobs, uint32_t max_cw, uint32_t max_ch, bool all_rgba_aligned, hipStream_t st)
{
    if (all_rgba_aligned) {
        dim3 gridf((max_cw * max_ch + 255u) / 256u, njobs);
        hipLaunchKernelGGL(webp420_rgba_kernel, gridf, dim3(256), 0, st, fjobs, arena, gamma_off, job_base);
        return hipGetLastError();
    }
    dim3 grid((max_cw + 255u) / 256u, max_ch, njobs);
    hipLaunchKernelGGL(webp420_kernel, grid, dim3(256), 0, st, fjobs, arena, gamma_off, job_base);
    return hipGetLastError();
}

} // namespace fl
