// fl_vp8_variant.h -- which lossy WebP front end is which.  The eight front ends are a cube of three switches: i4 (a macroblock's
// luma may be B_PRED), ap (per-picture coefficient probabilities), lf (a loop filter level picked on the device).  This is the one
// place that knows their codes; everything else asks for the variant.  Host only.
#pragma once
#include <stdint.h>

#include <optional>

#include "../../include/fanlin_gpu.h"

namespace fl {

struct Vp8Variant { bool i4, ap, lf; };

// The family of a launch: i4 | ap << 1 | lf << 2.  A batch's jobs are grouped by front end in ascending code, and launch_vp8_encode
// takes one range of jobs per family in ascending family, so the two orders must agree (asserted below).
constexpr uint32_t vp8_family(Vp8Variant v) { return (uint32_t)v.i4 | (uint32_t)v.ap << 1 | (uint32_t)v.lf << 2; }
constexpr Vp8Variant vp8_variant_of_family(uint32_t f) { return Vp8Variant{(f & 1u) != 0, (f & 2u) != 0, (f & 4u) != 0}; }

constexpr uint32_t vp8_front_end(Vp8Variant v)
{
    return v.lf ? FLGPU_FE_WEBP_LOSSY_LF + (vp8_family(v) & 3u) : (v.ap ? FLGPU_FE_WEBP_LOSSY_AP : FLGPU_FE_WEBP_LOSSY) + (uint32_t)v.i4;
}
// the variant of a front end, or nothing: not a lossy WebP front end
constexpr std::optional<Vp8Variant> vp8_variant_of(uint32_t front_end)
{
    if (front_end < FLGPU_FE_WEBP_LOSSY || front_end > FLGPU_FE_WEBP_LOSSY_I4_AP_LF) return std::nullopt; // (every other front end leaves here)
    for (uint32_t f = 0; f < 8u; ++f)
        if (vp8_front_end(vp8_variant_of_family(f)) == front_end) return vp8_variant_of_family(f);
    return std::nullopt;
}

static_assert(vp8_front_end({false, false, false}) == FLGPU_FE_WEBP_LOSSY && FLGPU_FE_WEBP_LOSSY == 9 &&
              vp8_front_end({true, false, false}) == FLGPU_FE_WEBP_LOSSY_I4 && FLGPU_FE_WEBP_LOSSY_I4 == 10 &&
              vp8_front_end({false, true, false}) == FLGPU_FE_WEBP_LOSSY_AP && FLGPU_FE_WEBP_LOSSY_AP == 12 &&
              vp8_front_end({true, true, false}) == FLGPU_FE_WEBP_LOSSY_I4_AP && FLGPU_FE_WEBP_LOSSY_I4_AP == 13 &&
              vp8_front_end({false, false, true}) == FLGPU_FE_WEBP_LOSSY_LF && FLGPU_FE_WEBP_LOSSY_LF == 16 &&
              vp8_front_end({true, false, true}) == FLGPU_FE_WEBP_LOSSY_I4_LF && FLGPU_FE_WEBP_LOSSY_I4_LF == 17 &&
              vp8_front_end({false, true, true}) == FLGPU_FE_WEBP_LOSSY_AP_LF && FLGPU_FE_WEBP_LOSSY_AP_LF == 18 &&
              vp8_front_end({true, true, true}) == FLGPU_FE_WEBP_LOSSY_I4_AP_LF && FLGPU_FE_WEBP_LOSSY_I4_AP_LF == 19,
              "the codes of the eight front ends");
constexpr bool vp8_families_follow_their_codes()
{
    for (uint32_t f = 0; f < 8u; ++f) {
        const std::optional<Vp8Variant> v = vp8_variant_of(vp8_front_end(vp8_variant_of_family(f)));
        if (!v || vp8_family(*v) != f || (f && vp8_front_end(vp8_variant_of_family(f - 1u)) >= vp8_front_end(*v))) return false;
    }
    return !vp8_variant_of(11) && !vp8_variant_of(14) && !vp8_variant_of(15) && !vp8_variant_of(20);
}
static_assert(vp8_families_follow_their_codes(), "the decode inverts vp8_front_end, and family order is front-end order");

} // namespace fl
