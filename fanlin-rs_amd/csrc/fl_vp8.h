// fl_vp8.h -- the lossy WebP encoder (fl_vp8.hip; the opt-in front ends of fl_vp8_variant.h's Vp8Variant): job descriptor, scratch sizes and the launch.
// The format's limits and worst case (one rule over i4, ap, seg), and everything the kernels compute, are in fl_vp8_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_vp8_core.h"
#include "fl_vp8_lf_core.h"
#include "fl_webpll.h"

namespace fl {

constexpr uint32_t kVp8ResultAlphaVp8l = 2; // Vp8Job::result[0]
constexpr uint32_t kVp8ResultSegments = 4;  // Vp8Job::result[0]
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
    uint32_t *result;     // [0] bit 0: some pixel is not opaque, bit 1 (kVp8ResultAlphaVp8l): the ALPH chunk went out compressed, bit 2 (kVp8ResultSegments): the frame went out segmented; [1] = file bytes (0 if it did not fit dst_cap): the words and protocol of JpegJob
    uint32_t *bm;         // scratch, the I4 variants only (else nullptr): two words of sub-block modes per macroblock
    uint32_t w, h, c;
    uint32_t dst_cap;     // bytes available at dst
    uint32_t qi;          // quantiser index (vp8_quality_index of the clamped quality)
    int32_t lf_base;      // the loop-filtered variants: -1 = the base level from qi, 0..63 = forced (flgpu_debug_set "vp8_filter_base")
    uint8_t *tab;         // scratch, the adaptive-probability variants only (else nullptr): the picture's table, kVp8TabBytes
    uint8_t *lf;          // scratch, the loop-filtered variants only (else nullptr): four 64-bit cost words (kVp8LfCostBytes), then
                          // three working copies of the reconstruction, vp8_rec_bytes rounded up to 256 each
    const uint32_t *alpha; // FLGPU_FEO_ALPHA_VP8L only (else nullptr): what the alpha coder left (fl_webpll.h, an alpha-mode WebpJob::dst) where
                          // bit 0 of result[0] is set -- the stream's bytes, the stream from byte kWebpllAlphaHead on
    uint8_t *seg;         // scratch, FLGPU_FEO_SEGMENTS only (else nullptr): the picture's Vp8SegRec, then from byte kVp8SegHead on one
                          // byte per macroblock (vp8_seg_bytes): its activity bin while vp8_segment_kernel runs, its class after it
};
static_assert(sizeof(Vp8Job) == 128, "the job record: 96 bytes before the loop-filtered variants, their scratch pointer, the alpha coder's result, the segment scratch (and 8 of alignment)");

inline uint64_t vp8_planes_bytes(uint64_t w, uint64_t h) { return 2u * w * h + 2u * ((w + 1u) / 2u) * ((h + 1u) / 2u); }

constexpr uint32_t kVp8TabBytes = 4 * 8 * 3 * 11; // the coefficient probability table of one picture
// The families of a launch: f = i4 | ap << 1 | lf << 2 (fl_vp8_variant.h vp8_family), which is the order of their front ends and
// so of their jobs.
constexpr uint32_t kVp8Families = 8;
// scratch of one loop-filtered picture behind Vp8Job::lf
inline uint64_t vp8_lf_bytes(uint32_t mbw, uint32_t mbh) { return kVp8LfCostBytes + (kVp8LfCandidates - 1u) * ((vp8_rec_bytes(mbw, mbh) + 255u) & ~(uint64_t)255u); }

// predict / transform / quantise / reconstruct -> (the adaptive variants: token statistics and the picture's table ->) partition
// (the loop-filtered variants: candidate levels filtered and measured ->) sizes -> framing and alpha plane -> partitions; four to
// six stream-ordered launches per family that has pictures: n[f] jobs of family f, one range after the other.  The alpha coder's
// launches for jobs with Vp8Job::alpha (launch_webpll_encode, alpha mode) go before this call, after the planes launch.
// segmented: how many jobs have Vp8Job::seg; if any, one more launch goes in front of the families' (vp8_segment_kernel over all jobs).
hipError_t launch_vp8_encode(const Vp8Job *jobs, const uint32_t n[kVp8Families], hipStream_t st, uint32_t segmented = 0);

} // namespace fl
