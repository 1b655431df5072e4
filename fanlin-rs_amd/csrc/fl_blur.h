// fl_blur.h -- sizing rules of blur_tile_kernel (fl_blur.hip): lanes per workgroup, column tiles, rows per band and LDS bytes.
// Plain C++ that compiles for the host alone as well, so that a host-only program can hold build_blur_plan (fl_tables.cpp)
// against the kernel's LDS layout (tests/tools/asan_blur_plan.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FL_BLUR_HD __host__ __device__
#else
#define FL_BLUR_HD
#endif

namespace fl {

constexpr int BLUR_TY = 8;        // output rows per workgroup (colour)
constexpr int BLUR_TY_MONO = 8;   // ... when one channel is filtered (16 measured slower: 0.80 vs 0.61 ms, more zero-weight FMAs per band)
FL_BLUR_HD inline int blur_ty(uint32_t channels_filtered) { return channels_filtered == 1 ? BLUR_TY_MONO : BLUR_TY; }
constexpr uint32_t BLUR_MAXTAPS = 128;            // sigma <= 20 gives 81 taps
FL_BLUR_HD constexpr uint32_t blur_midw(uint32_t threads) { return threads + BLUR_MAXTAPS; } // columns of the f32 hand-off rows in LDS

FL_BLUR_HD inline uint32_t blur_tiles_t(uint32_t w, uint32_t taps, uint32_t threads) { const uint32_t cap = threads - (taps - 1); return (w + cap - 1) / cap; }
// Lanes per workgroup: a tile of tw output columns needs tw + taps - 1 lanes in the vertical pass, so the width that
// wastes the fewest lane slots wins (300 columns, 41 taps: 1 tile of 384 lanes instead of 2 of 256)
FL_BLUR_HD inline uint32_t blur_threads(uint32_t w, uint32_t taps)
{
    uint32_t best = 256, cost = 0xffffffffu;
    for (uint32_t t = 256; t <= 512; t += 128) {
        const uint32_t c = blur_tiles_t(w, taps, t) * t;
        if (c < cost) { cost = c; best = t; }
    }
    return best;
}
FL_BLUR_HD inline uint32_t blur_tiles(uint32_t w, uint32_t taps) { return blur_tiles_t(w, taps, blur_threads(w, taps)); }

// Dynamic LDS of one workgroup, an upper bound over the picture's bands and tiles: the kernel lays out
// [ wv: rv x TY, rounded up to 4 floats | mid: TY x blur_midw(lanes) x MS | wh: htaps x nrows_h ] with rv <= TY + vtaps - 1
// source rows per band and nrows_h <= min(w, 2 htaps) distinct horizontal weight vectors (build_blur_plan).
inline size_t blur_lds_bytes_of(uint32_t w, uint32_t channels, uint32_t vtaps, uint32_t htaps)
{
    const size_t ty = (size_t)blur_ty(channels);
    const uint32_t ms = channels == 3 ? 4 : channels; // floats per pixel in LDS
    const size_t wv = ((ty + vtaps) * ty + 3) & ~(size_t)3;
    const size_t rows_h = w < 2 * (size_t)htaps ? w : 2 * (size_t)htaps; // <= htaps (borders) + 1 (interior)
    return (wv + ty * blur_midw(blur_threads(w, htaps)) * ms + (size_t)htaps * rows_h) * sizeof(float);
}

} // namespace fl
