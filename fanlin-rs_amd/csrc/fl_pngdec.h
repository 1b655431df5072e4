// fl_pngdec.h -- device half of the PNG decode front end (fl_pngdec.hip): undoing the row filters, and expanding palette,
// sub-byte and tRNS pictures to the pixels Transformations::EXPAND gives the image crate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_pngsrc.h"

namespace fl {

// Shape of png_unfilter_kernel: one workgroup per picture, kPdWaves waves; a wave owns a band of kPdBandRows consecutive
// rows (lane r = row r of the band, one pixel per step, r steps behind the row above it) and walks it in chunks of
// kPdChunk steps.  Band b runs on wave b % kPdWaves, kPdLag chunk steps behind band b - 1.
constexpr uint32_t kPdWaves = 8, kPdBandRows = 64, kPdChunk = 64, kPdLag = 2;
constexpr uint32_t kPdThreads = kPdWaves * 64u;
// LDS of a wave: its band's slice of the current chunk, one row per lane; the pitch in dwords is odd, so that the 64 lanes'
// reads of one step fall into 64 different banks
__host__ __device__ constexpr uint32_t png_lds_pitch(uint32_t bpp) { return kPdChunk * bpp + 4u; }
__host__ __device__ constexpr uint32_t png_lds_bytes(uint32_t bpp) { return kPdWaves * kPdBandRows * png_lds_pitch(bpp); }

// One picture of a decode launch.  An Adam7 picture is up to seven pictures to the unfilter kernel, one job per non-empty pass: the
// pass's width, height and row_bytes, its scanlines scan_off bytes into the stream, its own slice of the row scratch (adam7_pass).
// To the de-interlace kernel it is one job again: the whole picture's width and height, rows = where pass 1's rows begin.
struct alignas(16) PngDecJob {
    const uint8_t *blob;  // device copy: PngBlobHeader + filtered scanlines
    uint8_t *rows;        // unfiltered rows, pitch row_bytes: the pixels themselves (direct pictures) or the expand kernel's input
    uint8_t *pixels;      // width * height * channels, tightly packed (== rows for direct pictures)
    uint32_t width, height;
    uint32_t row_bytes, bpp;
    uint32_t scan_off;    // unfilter: where this job's scanlines begin behind the header (0 but for the passes of an Adam7 picture)
    uint32_t pad[3];
};

// njobs_bpp[k] jobs with bpp k + 1, in that order, starting at jobs[0]
hipError_t launch_png_unfilter(const PngDecJob *jobs, const uint32_t njobs_bpp[4], hipStream_t st);
// the jobs that need it; max_pixels = the largest width * height among them
hipError_t launch_png_expand(const PngDecJob *jobs, uint32_t njobs, uint32_t max_pixels, hipStream_t st);
// the Adam7 pictures, after their passes' unfilter jobs: the seven reduced pictures put together and expanded in one step
hipError_t launch_png_adam7(const PngDecJob *jobs, uint32_t njobs, uint32_t max_pixels, hipStream_t st);

} // namespace fl
