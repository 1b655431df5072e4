// fl_vp8.h -- the lossy WebP encoder (fl_vp8.hip; opt-in FLGPU_FE_WEBP_LOSSY, _I4, _AP and _I4_AP): job descriptor, scratch sizes and the launch.
// The format's limits and worst case, and everything the kernels compute, are in fl_vp8_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_vp8_core.h"

namespace fl {

constexpr uint32_t kVp8SizeWords = 12;  // per-picture scratch words: the sizes of partition 0 and of up to 8 token partitions

// One picture of a lossy-WebP launch.  The planes launch of FLGPU_FE_WEBP420 has written src (scratch here, not the caller's dst)
// and bit 0 of result[0].
struct alignas(16) Vp8Job {
    const uint8_t *src;   // Y | U | V | A planes, w x h luma, ceil(w / 2) x ceil(h / 2) chroma
    uint8_t *dst;         // the WebP file
    uint8_t *rec;         // scratch: the reconstruction, vp8_rec_bytes
    int16_t *lev;         // scratch: kVp8MbLevels levels per macroblock
    uint32_t *info;       // scratch: one record per macroblock
    uint32_t *sizes;      // scratch: [kVp8SizeWords]
    uint32_t *result;     // [0] bit 0: some pixel is not opaque; [1] = file bytes (0 if it did not fit dst_cap): the words and protocol of JpegJob
    uint32_t *bm;         // scratch, FLGPU_FE_WEBP_LOSSY_I4 only (else nullptr): two words of sub-block modes per macroblock
    uint32_t w, h, c;
    uint32_t dst_cap;     // bytes available at dst
    uint32_t qi;          // quantiser index (vp8_quality_index of the clamped quality)
    uint32_t pad[1];
    uint8_t *tab;         // scratch, the adaptive-probability variants only (else nullptr): the picture's table, kVp8TabBytes
};
static_assert(sizeof(Vp8Job) == 96, "the job record keeps its size");

inline uint64_t vp8_planes_bytes(uint64_t w, uint64_t h) { return 2u * w * h + 2u * ((w + 1u) / 2u) * ((h + 1u) / 2u); }

constexpr uint32_t kVp8TabBytes = 4 * 8 * 3 * 11; // the coefficient probability table of one picture
// The families of a launch in the order of their front ends, which is the order of their jobs: FLGPU_FE_WEBP_LOSSY, _I4, _AP, _I4_AP.
constexpr uint32_t kVp8Families = 4;
constexpr uint32_t vp8_family(uint32_t front_end) { return front_end == 9u ? 0u : front_end == 10u ? 1u : front_end == 12u ? 2u : 3u; }

// predict / transform / quantise / reconstruct -> (the adaptive variants: token statistics and the picture's table ->) partition
// sizes -> framing and alpha plane -> partitions; four or five stream-ordered launches per family that has pictures: n[f] jobs of
// family f, one range after the other
hipError_t launch_vp8_encode(const Vp8Job *jobs, const uint32_t n[kVp8Families], hipStream_t st);

} // namespace fl
