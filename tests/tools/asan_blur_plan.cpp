// Host-only harness for tests/test_blur_plan_host.py: blur_tile_kernel's table block (csrc/fl_tables.cpp build_blur_plan) against what the
// kernel (csrc/fl_blur.hip) relies on when it reads it -- the lane count and the LDS bytes of csrc/fl_blur.h -- over a sweep of sigmas,
// widths and heights, built with -fsanitize=address,undefined.  Any violated invariant prints the case and ends the run with status 1.
// Prints "<plans> <refused> <plans at 256 lanes> <at 384> <at 512>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fl_blur.h"
#include "fl_tables.h"
#include "fl_types.h"

using namespace fl;

static const float kSigmas[] = {0.3f, 0.5f, 1.0f, 2.5f, 3.0f, 5.0f, 10.0f, 10.5f, 14.3f, 20.0f, 24.0f, 28.0f, 30.0f, 31.75f};
static const uint32_t kWidths[] = {1, 2, 3, 7, 41, 81, 136, 137, 176, 177, 216, 217, 256, 257, 304, 305, 352, 353, 432, 433, 472, 473, 640, 700, 900, 1297, 2000};
static const uint32_t kHeights[] = {1, 7, 8, 9, 12, 13, 61, 90};

static float sigma_now;
static uint32_t w_now, h_now;
static int failures;

#define CHECK(cond, ...)                                                                              \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            fprintf(stderr, "sigma %g, %u x %u: %s: ", (double)sigma_now, w_now, h_now, #cond);       \
            fprintf(stderr, __VA_ARGS__);                                                             \
            fprintf(stderr, "\n");                                                                    \
            if (++failures > 20) return;                                                              \
        }                                                                                             \
    } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static void check_plan(const HostAxis &v, const HostAxis &h, uint32_t ty, uint32_t lanes)
{
    const uint32_t w = h.out_size, hh = v.out_size, htaps = h.max_taps, vtaps = v.max_taps;
    const uint32_t nt = blur_tiles(w, htaps);
    std::vector<uint32_t> blk;
    build_blur_plan(v, h, nt, ty, blk);
    CHECK(blk.size() >= sizeof(BlurPlanHeader) / 4, "%zu words", blk.size());
    BlurPlanHeader hd;
    memcpy(&hd, blk.data(), sizeof(hd));
    // the header, and every area inside the block
    CHECK(hd.nt == nt && hd.nb == (hh + ty - 1) / ty && hd.htaps == htaps, "nt %u nb %u htaps %u", hd.nt, hd.nb, hd.htaps);
    CHECK(hd.tw_full >= 1 && hd.tw_full <= lanes, "tw_full %u, %u lanes", hd.tw_full, lanes);
    CHECK((uint64_t)hd.tw_full * nt >= w, "tiles of %u columns x %u do not cover the width", hd.tw_full, nt);
    CHECK(hd.tiles_off >= sizeof(BlurPlanHeader) / 4 && hd.tiles_off + 2 * nt <= hd.bands_off && hd.bands_off + 2 * hd.nb <= hd.vdense_off &&
              hd.vdense_off % 4 == 0 && (uint64_t)hd.vdense_off + (uint64_t)hd.nb * hd.rv * ty <= hd.htiles_off &&
              (uint64_t)hd.htiles_off + (uint64_t)nt * hd.tw_full * 2 <= hd.hrows_off && (uint64_t)hd.hrows_off + (uint64_t)htaps * hd.nrows_h == blk.size(),
          "areas overlap or leave the block of %zu words", blk.size());
    if (failures) return;
    CHECK(hd.rv <= ty + vtaps - 1, "rv %u, ty %u, vtaps %u", hd.rv, ty, vtaps);
    CHECK(hd.nrows_h >= 1 && hd.nrows_h <= std::min<uint64_t>(w, 2 * (uint64_t)htaps), "nrows_h %u, htaps %u", hd.nrows_h, htaps);
    // the three LDS areas as the kernel lays them out, for every channel count that shares this band height
    for (uint32_t ch = 1; ch <= 4; ++ch) {
        if ((uint32_t)blur_ty(ch) != ty) continue;
        const uint64_t ms = ch == 3 ? 4 : ch;
        const uint64_t wv_floats = ((uint64_t)hd.rv * ty + 3u) & ~(uint64_t)3u;
        const uint64_t floats = wv_floats + (uint64_t)ty * blur_midw(lanes) * ms + (uint64_t)htaps * hd.nrows_h;
        CHECK(floats * 4 <= blur_lds_bytes_of(w, ch, vtaps, htaps), "%u channels: the kernel lays out %llu bytes, blur_lds_bytes() says %zu", ch,
              (unsigned long long)floats * 4, blur_lds_bytes_of(w, ch, vtaps, htaps));
    }
    // column tiles: the vertical pass has one lane per source column; the horizontal pass reads htaps hand-off columns from hleft on
    const uint32_t *tiles = blk.data() + hd.tiles_off, *bands = blk.data() + hd.bands_off;
    const float *hr = reinterpret_cast<const float *>(blk.data() + hd.hrows_off);
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t x0 = t * hd.tw_full;
        if (x0 >= w) { CHECK(tiles[2 * t + 1] == 0, "tile %u past the picture has %u columns", t, tiles[2 * t + 1]); continue; }
        const uint32_t cl = tiles[2 * t], ncols = tiles[2 * t + 1], tw = std::min(hd.tw_full, w - x0);
        CHECK(ncols >= 1 && ncols <= lanes, "tile %u: %u source columns, %u lanes", t, ncols, lanes);
        CHECK((uint64_t)cl + ncols <= w, "tile %u: source columns %u + %u", t, cl, ncols);
        const uint32_t *tt = blk.data() + hd.htiles_off + (size_t)t * hd.tw_full * 2;
        for (uint32_t j = 0; j < tw; ++j) {
            const uint32_t x = x0 + j, hleft = tt[2 * j], hrow = tt[2 * j + 1];
            CHECK(hleft + htaps <= blur_midw(lanes), "column %u: hleft %u + %u taps, hand-off row of %u", x, hleft, htaps, blur_midw(lanes));
            CHECK(cl + hleft == h.left[x] && hleft + h.count[x] <= ncols, "column %u: window %u + %u, tile loads %u + %u", x, cl + hleft, h.count[x], cl, ncols);
            CHECK(hrow < hd.nrows_h, "column %u: weight vector %u of %u", x, hrow, hd.nrows_h);
            for (uint32_t i = 0; i < htaps; ++i) {
                const float want = i < h.count[x] ? h.weights[h.woff[x] + i] : 0.0f;
                CHECK(bits(hr[(size_t)i * hd.nrows_h + hrow]) == bits(want), "column %u tap %u: %g, axis %g", x, i, (double)hr[(size_t)i * hd.nrows_h + hrow], (double)want);
            }
        }
    }
    // row bands and their dense vertical weights
    const float *vd = reinterpret_cast<const float *>(blk.data() + hd.vdense_off);
    for (uint32_t b = 0; b < hd.nb; ++b) {
        const uint32_t top = bands[2 * b], nrows = bands[2 * b + 1], y0 = b * ty;
        CHECK(nrows >= 1 && nrows <= hd.rv && (uint64_t)top + nrows <= hh, "band %u: rows %u + %u, rv %u", b, top, nrows, hd.rv);
        for (uint32_t o = 0; o < ty; ++o)
            for (uint32_t r = 0; r < hd.rv; ++r) {
                const uint32_t y = y0 + o, row = top + r;
                float want = 0.0f;
                if (y < hh && row >= v.left[y] && row < v.left[y] + v.count[y]) want = v.weights[v.woff[y] + (row - v.left[y])];
                if (y < hh && r >= nrows) CHECK(want == 0.0f, "band %u: output row %u wants source row %u, the band stops at %u", b, y, row, top + nrows);
                CHECK(bits(vd[((size_t)b * hd.rv + r) * ty + o]) == bits(want), "band %u row %u output %u: %g, axis %g", b, r, o, (double)vd[((size_t)b * hd.rv + r) * ty + o], (double)want);
            }
    }
}

int main()
{
    unsigned plans = 0, refused = 0, at[3] = {0, 0, 0};
    std::vector<uint32_t> tys;
    for (uint32_t ch = 1; ch <= 4; ++ch)
        if (std::find(tys.begin(), tys.end(), (uint32_t)blur_ty(ch)) == tys.end()) tys.push_back((uint32_t)blur_ty(ch));
    for (float sigma : kSigmas)
        for (uint32_t w : kWidths) {
            HostAxis h;
            build_axis(w, w, FILTER_GAUSSIAN, sigma, h);
            for (uint32_t hh : kHeights) {
                HostAxis v;
                build_axis(hh, hh, FILTER_GAUSSIAN, sigma, v);
                sigma_now = sigma; w_now = w; h_now = hh;
                // what plan_blur / add_blur_launch (csrc/fl_batch.cpp) accept: blur_tile_supported() of both axes
                if (h.max_taps < 1 || h.max_taps > BLUR_MAXTAPS || v.max_taps < 1 || v.max_taps > BLUR_MAXTAPS) { ++refused; continue; }
                const uint32_t lanes = blur_threads(w, h.max_taps);
                if (lanes != 256 && lanes != 384 && lanes != 512) { fprintf(stderr, "sigma %g, width %u: %u lanes\n", (double)sigma, w, lanes); return 1; }
                for (uint32_t ty : tys) check_plan(v, h, ty, lanes);
                if (failures) return 1;
                ++plans;
                ++at[(lanes - 256) / 128];
            }
        }
    printf("%u %u %u %u %u\n", plans, refused, at[0], at[1], at[2]);
    return 0;
}
