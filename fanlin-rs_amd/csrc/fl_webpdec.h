// fl_webpdec.h -- device half of the lossless WebP decode front end (fl_webpdec.hip): the VP8L transforms inverted, last to
// first, on the residual picture the host half (fl_webpsrc.h) leaves, down to the interleaved R, G, B(, A) bytes the pipeline reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_webpsrc.h"

namespace fl {

// Shape of webp_predict_kernel: one workgroup per picture, kWdWaves waves; a wave owns a band of kWdBandRows consecutive rows
// (lane r = row r of the band, one pixel per step, 2 r steps behind the band's first row: a pixel needs its top-RIGHT
// neighbour) and walks it in chunks of kWdChunk steps.  Band b runs on wave b % kWdWaves, kWdLag chunk steps behind band b - 1:
// lane 0 of a band needs pixel 64 j + 64 of the row above it in chunk j, which lane 63 of the band above finishes at step
// 64 j + 64 + 126, in chunk j + 2.
constexpr uint32_t kWdWaves = 8, kWdBandRows = 64, kWdChunk = 64, kWdLag = 3;
constexpr uint32_t kWdThreads = kWdWaves * 64u;
constexpr uint32_t kWdSkew = 2u * (kWdBandRows - 1u); // steps between a band's first and last row
// LDS of a wave: its band's slice of the current chunk, one row per lane; the pitch in dwords is odd, so that the 64 lanes'
// accesses of one step fall into 64 different banks
constexpr uint32_t kWdPitch = kWdChunk + 1u; // dwords
constexpr uint32_t kWdLdsBytes = kWdWaves * kWdBandRows * kWdPitch * 4u;

// The predictor transform of one picture.
struct alignas(16) WebpPredictJob {
    const uint32_t *res;   // residuals, width x height dwords
    const uint32_t *modes; // mode image: ceil(width / 2^bits) dwords a row, the mode in the green byte
    uint32_t *out;         // width x height dwords
    uint32_t width, height, bits, pad;
};

// A run of pointwise inverse transforms in the order they are applied, read from `src` (src_w dwords a row) and written to
// `dst`: as dwords (out_c == 0, dst_w a row) or as out_c interleaved bytes R, G, B(, A).  Colour indexing inside a run widens
// the picture from src_w to dst_w; the operations in front of it run at the packed width.
struct WebpOp {
    uint32_t type;         // kWtCrossColor, kWtSubtractGreen (= add green), kWtColorIndexing
    uint32_t bits;         // cross-colour: block bits; colour indexing: the shift, pixels per green byte = 1 << shift
    uint32_t width;        // cross-colour: the width its blocks are laid out over
    uint32_t pad;
    const uint32_t *data;  // cross-colour: element image; colour indexing: 256-entry palette
};
struct alignas(16) WebpRunJob {
    const uint32_t *src;
    void *dst;
    uint32_t src_w, dst_w, height;
    uint32_t out_c;        // 0 = dwords, 3 / 4 = bytes
    uint32_t nops, shift;  // shift: of the colour indexing in this run (0 without one)
    WebpOp ops[4];
};

hipError_t launch_webp_predict(const WebpPredictJob *jobs, uint32_t njobs, hipStream_t st);
// max_pixels = the largest dst_w * height among the jobs
hipError_t launch_webp_run(const WebpRunJob *jobs, uint32_t njobs, uint32_t max_pixels, hipStream_t st);

} // namespace fl
