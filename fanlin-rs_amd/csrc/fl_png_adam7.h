// fl_png_adam7.h -- the pass geometry of Adam7-interlaced PNG files (PNG specification, 8.2), as code that compiles for the host and
// for the device: the host half (fl_pngsrc.cpp) sizes and checks the stream with it, the launch code (fl_source.cpp) cuts one
// unfilter job per pass from it, the de-interlace kernel (fl_pngdec.hip) finds a pixel's sample with it.  This is the one place that
// states the table; plain C++, no HIP needed.
//
// An interlaced picture is stored as seven reduced pictures back to back, pass p holding the pixels (x0 + i dx, y0 + j dy):
//
//   pass   1  2  3  4  5  6  7          the 8 x 8 tile, by pass:   1 6 4 6 2 6 4 6
//   x0     0  4  0  2  0  1  0                                     7 7 7 7 7 7 7 7
//   y0     0  0  4  0  2  0  1                                     5 6 5 6 5 6 5 6
//   dx     8  8  4  4  2  2  1                                     7 7 7 7 7 7 7 7
//   dy     8  8  8  4  4  2  2                                     3 6 4 6 3 6 4 6
//                                                                  7 7 7 7 7 7 7 7
//                                                                  5 6 5 6 5 6 5 6
//                                                                  7 7 7 7 7 7 7 7
//
// Every pass is a non-interlaced picture of its own: a filter byte in front of each of its rows, each row packed on its own (a
// sub-byte row ends with its own padding bits), its first row has no row above.  A pass of zero width or zero height is absent.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FL_A7_HD __host__ __device__ inline
#else
#define FL_A7_HD inline
#endif

namespace fl {

constexpr uint32_t kAdam7Passes = 7;

// The table above, a nibble per pass (pass 1 in the lowest): the origins, and the steps as shifts.  Passes are numbered from 0 here.
struct Adam7Geom { uint32_t x0, y0, sx, sy; }; // dx = 1 << sx, dy = 1 << sy
FL_A7_HD constexpr Adam7Geom adam7_geom(uint32_t p)
{
    return Adam7Geom{(0x0102040u >> (4u * p)) & 15u, (0x1020400u >> (4u * p)) & 15u, (0x0112233u >> (4u * p)) & 15u, (0x1122333u >> (4u * p)) & 15u};
}

// The pass of pixel (x & 7, y & 7), at [8 * (y & 7) + (x & 7)]: derived from adam7_geom, not restated.
struct Adam7Map { uint8_t pass[64]; };
constexpr Adam7Map adam7_map()
{
    Adam7Map m{};
    for (uint32_t y = 0; y < 8; ++y)
        for (uint32_t x = 0; x < 8; ++x)
            for (uint32_t p = 0; p < kAdam7Passes; ++p) {
                const Adam7Geom g = adam7_geom(p);
                if (x >= g.x0 && y >= g.y0 && ((x - g.x0) & ((1u << g.sx) - 1u)) == 0u && ((y - g.y0) & ((1u << g.sy) - 1u)) == 0u) m.pass[8u * y + x] = (uint8_t)p;
            }
    return m;
}

// One pass of a width x height picture of pixel_bits (samples x depth) bits per pixel.
struct Adam7Pass {
    uint32_t w, h;        // of the reduced picture: ceil((width - x0) / dx), or 0 if width <= x0; h likewise.  Absent if either is 0
    uint32_t row_bytes;   // ceil(w * pixel_bits / 8): a pass row without its filter byte
    uint64_t scan_off;    // of the pass's first filter byte in the inflated stream: the sum of h x (1 + row_bytes) of the passes before it
    uint64_t rows_off;    // the same without the filter bytes: where the pass's unfiltered rows go, tightly packed pass after pass
};
// (the loop runs over all seven passes whatever p is: on the device every lane takes the same number of steps)
FL_A7_HD Adam7Pass adam7_pass(uint32_t width, uint32_t height, uint32_t pixel_bits, uint32_t p)
{
    Adam7Pass out{0, 0, 0, 0, 0};
    for (uint32_t q = 0; q < kAdam7Passes; ++q) {
        const Adam7Geom g = adam7_geom(q);
        const uint32_t w = width > g.x0 ? (width - g.x0 + (1u << g.sx) - 1u) >> g.sx : 0u;
        const uint32_t h = height > g.y0 ? (height - g.y0 + (1u << g.sy) - 1u) >> g.sy : 0u;
        const uint64_t rb = ((uint64_t)w * pixel_bits + 7u) / 8u;   // (sides are below 2^31 and pixel_bits at most 32: the sums stay below 2^64)
        const uint64_t rows = (w && h) ? (uint64_t)h * rb : 0u, scan = (w && h) ? (uint64_t)h * (1u + rb) : 0u;
        if (q < p) { out.scan_off += scan; out.rows_off += rows; }
        if (q == p) { out.w = w; out.h = h; out.row_bytes = rb <= 0xffffffffu ? (uint32_t)rb : 0u; } // (0: a picture the size bound refuses)
    }
    return out;
}
// Bytes of the whole inflated stream (p = 7: every pass lies in front) and of the unfiltered rows.
FL_A7_HD uint64_t adam7_scan_bytes(uint32_t width, uint32_t height, uint32_t pixel_bits) { return adam7_pass(width, height, pixel_bits, kAdam7Passes).scan_off; }
FL_A7_HD uint64_t adam7_rows_bytes(uint32_t width, uint32_t height, uint32_t pixel_bits) { return adam7_pass(width, height, pixel_bits, kAdam7Passes).rows_off; }

} // namespace fl
