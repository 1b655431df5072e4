// fl_gif_quant_core.h -- the colour quantiser behind FLGPU_ENCODE_GIF_QUANTIZE (fl_gifquant.hip): the rule's arithmetic as code that
// compiles for the host and for the device.  tests/gif_quant_model.py restates the rule, tests/gif_quant_host.cpp runs these
// functions in plain loops.  The rule is this project's own -- a variance-ordered median cut over a histogram whose precision follows
// the frame -- and nothing of the reference's NeuQuant is restated.
//
// The rule, integer only, for a frame whose distinct keys (r, g, b, alpha as 0 / 255) exceed 256:
//   * alpha != 0 is opaque.  Any alpha-0 pixel reserves one entry behind the opaque ones: K = 255, else K = 256.
//   * s = the least of 0, 1, 2, 3 at which the opaque pixels have at most kGifQuantHashCells distinct (r >> s, g >> s, b >> s);
//     3 if none has (at most 32,768 cells, indexed directly).
//   * one cell per distinct reduced colour: n and the sums of the exact samples; representative c = (sum + n / 2) / n per channel.
//   * boxes of cells: N = sum n, per axis S = sum n c, Q = sum n c c, V = N Q - S S in 64 bits.  A box's axis is the one of greatest
//     V (r before g before b), its priority V / N, its cut t = S / N on that axis; it is splittable iff V > 0.  While there are
//     fewer than K boxes: the splittable box of greatest priority (lowest number on ties) hands its cells with c[axis] > t to box
//     number `boxes`.  V > 0 leaves neither half empty.
//   * entry of a box = (exact sums + N / 2) / N; entries ascending by (r, g, b, box number); the transparent entry (0, 0, 0) behind.
//   * an opaque pixel takes the entry of least dr^2 + dg^2 + db^2 on its exact samples, the lowest index on ties.
// N Q and S S stay below 2^60 for frames of at most kGifQuantMaxPixels pixels; larger frames are not quantised.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FL_GQ_HD __host__ __device__ inline
#else
#define FL_GQ_HD inline
#endif

namespace fl {

constexpr uint32_t kGifQuantMaxPixels = 1u << 22;
constexpr uint32_t kGifQuantHashCells = 4096;   // distinct reduced colours at s = 0, 1, 2
constexpr uint32_t kGifQuantHashSlots = 8192;   // open addressing: the cells and at most one key per thread in flight
constexpr uint32_t kGifQuantCells = 32768;      // cells of a frame at most: the direct table of s = 3; a frame's scratch arrays
constexpr uint32_t kGifQuantNoCell = 0xffffffffu;

// what the frame record's eighth word holds for a marked frame, as the kernels go: the mark, then s, then whether a pixel is clear
constexpr uint32_t kGqMarked = 1u, kGqShift = 4u /* s << 4 */, kGqClear = 0x100u;

// (r >> s, g >> s, b >> s) of a key (r, g, b, a big-endian) in 24 bits; at s = 3 the 15-bit cell number instead
FL_GQ_HD uint32_t gq_reduced(uint32_t key, uint32_t s) { return ((key >> 24) >> s) << 16 | (((key >> 16) & 255u) >> s) << 8 | (((key >> 8) & 255u) >> s); }
FL_GQ_HD uint32_t gq_cell15(uint32_t key) { return (key >> 27) << 10 | ((key >> 19) & 31u) << 5 | ((key >> 11) & 31u); }

// representative of a cell, entry of a box: the rounded mean of the exact samples
FL_GQ_HD uint32_t gq_mean(uint32_t sum, uint32_t n) { return (sum + n / 2u) / n; }
FL_GQ_HD uint32_t gq_pack(uint32_t r, uint32_t g, uint32_t b) { return r << 16 | g << 8 | b; }
FL_GQ_HD uint32_t gq_axis_of(uint32_t packed, uint32_t axis) { return (packed >> (16u - 8u * axis)) & 255u; }

struct GqBox {
    uint64_t q[3]; // sum n c c
    uint32_t s[3]; // sum n c  (below 2^30)
    uint32_t n;
};
FL_GQ_HD void gq_box_clear(GqBox &b) { b.n = 0; for (int a = 0; a < 3; ++a) { b.s[a] = 0; b.q[a] = 0; } }
FL_GQ_HD void gq_box_add(GqBox &b, uint32_t n, uint32_t packed)
{
    b.n += n;
    for (uint32_t a = 0; a < 3u; ++a) { const uint32_t c = gq_axis_of(packed, a), nc = n * c; b.s[a] += nc; b.q[a] += (uint64_t)nc * c; }
}
FL_GQ_HD void gq_box_merge(GqBox &b, const GqBox &o) { b.n += o.n; for (int a = 0; a < 3; ++a) { b.s[a] += o.s[a]; b.q[a] += o.q[a]; } }
FL_GQ_HD void gq_box_remove(GqBox &b, const GqBox &o) { b.n -= o.n; for (int a = 0; a < 3; ++a) { b.s[a] -= o.s[a]; b.q[a] -= o.q[a]; } }

// what the split loop asks of a box: rank = 0 if it cannot be split, else priority + 1 (priority < 2^39)
struct GqChoice { uint64_t rank; uint32_t axis, cut; };
FL_GQ_HD GqChoice gq_choice(const GqBox &b)
{
    GqChoice c = {0u, 0u, 0u};
    if (!b.n) return c;
    uint64_t best = 0;
    for (uint32_t a = 0; a < 3u; ++a) {
        const uint64_t v = (uint64_t)b.n * b.q[a] - (uint64_t)b.s[a] * b.s[a];
        if (v > best) { best = v; c.axis = a; } // (strictly greater: r before g before b)
    }
    c.cut = b.s[c.axis] / b.n;
    c.rank = best ? best / b.n + 1u : 0u;
    return c;
}
// the greater of two (rank, box) pairs in one word: the higher rank, on ties the lower box number
FL_GQ_HD uint64_t gq_select_word(uint64_t rank, uint32_t box) { return rank ? rank << 8 | (255u - box) : 0u; }
FL_GQ_HD uint32_t gq_selected_box(uint64_t word) { return 255u - (uint32_t)(word & 255u); }

// keys as fl_gif.hip makes them: r, g, b, a big-endian in a dword, alpha normalised to 0 / 255 (LumaA8 as l, l, l, a)
FL_GQ_HD uint32_t gq_key_rgba(uint32_t v) { return (__builtin_bswap32(v) & 0xffffff00u) | ((v >> 24) ? 255u : 0u); }
FL_GQ_HD uint32_t gq_key_la(uint32_t v) { return (v & 255u) * 0x01010100u | ((v >> 8) ? 255u : 0u); }

// one step of the nearest-entry search: entry number i (packed) against the pixel of `key`; strictly nearer wins, so the lowest index keeps a tie
FL_GQ_HD void gq_nearer(uint32_t entry, uint32_t i, uint32_t key, uint32_t &best, uint32_t &at)
{
    const int32_t dr = (int32_t)(key >> 24) - (int32_t)(entry >> 16), dg = (int32_t)((key >> 16) & 255u) - (int32_t)((entry >> 8) & 255u),
                  db = (int32_t)((key >> 8) & 255u) - (int32_t)(entry & 255u);
    const uint32_t d = (uint32_t)(dr * dr + dg * dg + db * db);
    if (d < best) { best = d; at = i; }
}
// the index of the entry nearest to the opaque pixel of `key` among table[0 .. n), n >= 1
FL_GQ_HD uint32_t gq_nearest(const uint32_t *table, uint32_t n, uint32_t key)
{
    uint32_t best = 0xffffffffu, at = 0u;
    for (uint32_t i = 0; i < n; ++i) gq_nearer(table[i], i, key, best, at);
    return at;
}

} // namespace fl
