// fl_vp8dec.h -- device half of the lossy WebP decode front end (fl_vp8dec.hip): the levels and macroblock records the host half
// (fl_vp8src.h) leaves, through dequantisation, inverse transforms, intra prediction, the loop filter, the ALPH filters and
// libwebp's up-sampling and colour conversion, down to the interleaved R, G, B(, A) bytes the pipeline reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_vp8src.h"

namespace fl {

// Shape of vp8dec_recon_kernel and vp8dec_filter_kernel: one workgroup per picture; macroblock (x, y) needs its left, above,
// above-left and above-right neighbours, so the workgroup steps through the anti-diagonals d = x + 2 y, its waves take the
// macroblocks of a diagonal (reconstruction: one a wave; filter: two a wave, 32 lines each), and barriers separate the steps.
constexpr uint32_t kVp8dWaves = 16, kVp8dThreads = kVp8dWaves * 64u;
constexpr uint32_t kVp8dRgbThreads = 256, kVp8dRgbRun = 4; // vp8dec_rgb_kernel: pixels per thread

struct alignas(16) Vp8DecJob {
    const uint8_t *blob;  // device copy of what vp8_decode_levels left
    uint8_t *planes;      // vp8_rec_bytes(mbw, mbh): Y | U | V padded to whole macroblocks
    uint8_t *alpha;       // width x height, or nullptr for a picture without an ALPH plane
    const uint8_t *alpha_src; // the plane as the ALPH filter left it: in the blob (stride 1), or the green bytes of the R, G, B, A picture
    uint64_t alpha_stride;    // the lossless transforms wrote for a VP8L-coded plane (stride 4)
    uint8_t *dst;         // width x height x channels
    uint32_t width, height, channels, filtered; // filtered: the blob's filter_type != 0
};

// The jobs whose `filtered` is set come first: the filter kernel is launched for those alone (none: no launch).
// stage: 0 = everything; 1 = reconstruction only, 2 = reconstruction and loop filter (flgpu_debug_vp8_planes)
hipError_t launch_vp8_decode(const Vp8DecJob *jobs, const Vp8DecJob *host_jobs, uint32_t njobs, hipStream_t st, int stage = 0);

} // namespace fl
