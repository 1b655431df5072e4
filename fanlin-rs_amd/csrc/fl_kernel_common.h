// fl_kernel_common.h -- device helpers and launch dispatch shared by fl_resample.hip, fl_stream.hip, fl_place.hip and fl_blur.hip.
//
// Arithmetic contract of those kernels: every resample/blur tap is one fused f32 multiply-add applied in the
// reference's tap order (image 0.25.6 imageops/sample.rs: vertical pass first into an unrounded f32 image, then the horizontal
// pass, clamp, round half away from zero).  Everything else (grayscale, invert, overlay/fill, the colour kernels of fl_color.hip)
// is evaluated with the reference's own operation order and must match it bit for bit, so the tree is compiled with
// -ffp-contract=off and fuses only where __builtin_fmaf says so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "fl_pixel.h"
#include "fl_types.h"

namespace fl {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// image::color rgb_to_luma for u8: (2126 R + 7152 G + 722 B) / 10000, truncating (u32 maths).
__device__ __forceinline__ uint32_t luma_u8(uint32_t r, uint32_t g, uint32_t b)
{
    return (2126u * r + 7152u * g + 722u * b) / 10000u;
}

// FloatNearest + NumCast in horizontal_sample: clamp to [0,255], round half away from zero.
__device__ __forceinline__ uint32_t round_u8(float t)
{
    t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
    float f = __builtin_floorf(t);
    if (t - f >= 0.5f) f += 1.0f; // t - f is exact here
    return (uint32_t)f;
}

// One dword / byte to global memory, invisible to hipcc's s_waitcnt bookkeeping (see load_row in fl_stream.hip).
__device__ __forceinline__ void store_hidden_b32(void *p, uint32_t v)
{
    asm volatile("global_store_dword %0, %1, off\n\ts_nop 0" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store_hidden_b8(void *p, uint32_t v)
{
    asm volatile("global_store_byte %0, %1, off\n\ts_nop 0" : : "v"(p), "v"(v) : "memory");
}

// Writes one resampled pixel (MC rounded channels in c[]) to the destination.
// LB = letterboxed: destination is Rgba8, pixel converted with to_rgba() and blended onto the fill.
template <int MC, bool LB, bool HIDDEN = false>
__device__ __forceinline__ void store_pixel(uint8_t *dst, uint32_t pix_index, const uint32_t *c, uint32_t fill)
{
    if (LB) {
        uint32_t v;
        if (MC == 1) v = c[0] | (c[0] << 8) | (c[0] << 16) | (255u << 24);
        else if (MC == 2) v = blend_over_fill(fill, c[0], c[0], c[0], c[1]);
        else if (MC == 3) v = c[0] | (c[1] << 8) | (c[2] << 16) | (255u << 24);
        else v = blend_over_fill(fill, c[0], c[1], c[2], c[3]);
        if (HIDDEN) store_hidden_b32(reinterpret_cast<uint32_t *>(dst) + pix_index, v);
        else reinterpret_cast<uint32_t *>(dst)[pix_index] = v;
    } else {
        uint8_t *p = dst + (size_t)pix_index * MC;
#pragma unroll
        for (int k = 0; k < MC; ++k) {
            if (HIDDEN) store_hidden_b8(p + k, c[k]);
            else p[k] = (uint8_t)c[k];
        }
    }
}

// Applies the pre-op to one source pixel given as CS integer channels; writes MC floats.
template <int CS, int PRE>
__device__ __forceinline__ void preop_pixel(const uint32_t *s, float *v)
{
    if (PRE == PRE_GRAY && CS >= 3) {
        v[0] = (float)luma_u8(s[0], s[1], s[2]);
        if (CS == 4) v[1] = (float)s[3];
    } else if (PRE == PRE_INVERT) {
        constexpr int NC = (CS == 2 || CS == 4) ? CS - 1 : CS; // alpha is not inverted
#pragma unroll
        for (int k = 0; k < CS; ++k) v[k] = (float)(k < NC ? 255u - s[k] : s[k]);
    } else {
#pragma unroll
        for (int k = 0; k < CS; ++k) v[k] = (float)s[k];
    }
}

extern __shared__ __attribute__((aligned(16))) float fl_lds[];

// Workgroup barrier that orders LDS traffic only.
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Launch dispatch: runtime launch parameters become template arguments of a generic lambda.
template <class F> hipError_t dispatch_bool(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// f(integral_constant CS, integral_constant PRE) for the (source channels, pre-op) of a launch.  Grayscale of Luma / LumaA is the
// identity and the host maps it to PRE_NONE (fl_batch.cpp plan_pictures), so those pairs have no kernels.
template <class F> hipError_t dispatch_cs_pre(uint32_t cs, uint32_t pre, F &&f)
{
#define FL_CASE(C_, P_) if (cs == C_ && pre == P_) return f(std::integral_constant<int, C_>{}, std::integral_constant<int, P_>{})
    FL_CASE(1, PRE_NONE); FL_CASE(1, PRE_INVERT); FL_CASE(2, PRE_NONE); FL_CASE(2, PRE_INVERT);
    FL_CASE(3, PRE_NONE); FL_CASE(3, PRE_GRAY); FL_CASE(3, PRE_INVERT); FL_CASE(4, PRE_NONE); FL_CASE(4, PRE_GRAY); FL_CASE(4, PRE_INVERT);
#undef FL_CASE
    return hipErrorInvalidValue;
}

} // namespace fl
