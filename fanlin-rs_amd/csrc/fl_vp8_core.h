// fl_vp8_core.h -- the lossy WebP (VP8 key frame) encoder's arithmetic, as code that compiles for the host and for the device:
// quantiser set-up, intra prediction, forward / inverse transforms, the per-macroblock phases, the token walk, the boolean coder
// and the file layout.  fl_vp8.hip spreads the phases over the lanes of a wave; tests/vp8_host.cpp runs the same functions in
// plain loops, planes to file, on the CPU.  No HIP header is needed to include this one.
// The encoder's variants are three switches -- i4, ap, lf: fl_vp8_variant.h maps them to front ends -- and one option, seg; they are
// template axes of the coder below, and (i4, ap, seg) are the parameters of the one worst-case rule.
//
// The stream with every switch off (tests/vp8_model.py restates it in numpy): one key frame, every macroblock I16, luma and chroma
// mode each the one of DC / V / H / TM with the least integer SSE of prediction against source (ties: the first in that order),
// one segment, loop filter level 0, default coefficient probabilities, 1 / 2 / 4 / 8 token partitions, mb_no_coeff_skip with a
// per-picture probability.  Forward transforms and quantiser rounding are this encoder's own (integer only); everything the decoder repeats
// -- dequantisation, inverse WHT, inverse DCT, prediction, clamping -- is the format's.
//
// i4 (tests/vp8_i4_model.py restates it, fl_vp8_i4_core.h holds its analysis phases): the same stream, but a macroblock's luma may
// be B_PRED.  Per macroblock, in raster order:
//   1. I16 trial: the phases above.  S16 = the prediction SSE of the chosen luma mode.  Chroma is as above whatever follows.
//   2. I4 trial: the luma sub-blocks 0..15 in raster order.  Each forms the ten predictions B_DC, B_TM, B_VE, B_HE, B_LD, B_RD, B_VR,
//      B_VL, B_HD, B_HU (the format's numbering) from the reconstruction -- the macroblock's own sub-blocks before it, the row
//      above and the column to the left of the macroblock, borders and above-right as the decoder sees them (fl_vp8dec_core.h,
//      whose predictor it calls) --, takes the one with the least SSE against the source (ties: the lowest number), transforms the
//      residual, quantises all sixteen coefficients (DC: the y1_dc step, rounded to nearest; AC: the dead zone above), and
//      reconstructs as the decoder will into a working copy that the next sub-block predicts from.  S4 = the sum of the sixteen
//      chosen SSEs.
//   3. The macroblock is B_PRED iff S4 + vp8_i4_penalty(y1_ac) < S16.  (So a macroblock with S16 <= penalty needs no I4 trial.)
//   4. The chosen trial's levels, non-zero flags and reconstruction are the macroblock's; later macroblocks see only those.
// In partition 0 a B_PRED macroblock writes 0 for the luma tree's first boolean and its sixteen modes through the sub-block tree
// with kVp8BModeProb[above][left]; an I16 neighbour stands for DC -> B_DC, V -> B_VE, H -> B_HE, TM -> B_TM, outside the frame is
// B_DC.  Its tokens have no Y2 block, its luma blocks are type 3 from coefficient 0, it leaves the Y2 context of its column and
// row as it found them, and it is skipped when its 24 blocks are zero.
//
// ap (fl_vp8_ap_core.h states the rule, tests/vp8_ap_model.py restates it): the same macroblocks, levels and modes, but the
// picture's token-tree branches are counted first, a coefficient probability table is derived from the counts, partition 0 carries the
// updates (flag i is 1 and followed by the 8-bit probability where the picture's table differs from the default), and the token
// partitions are coded with that table.  The reconstruction does not change.
//
// lf (fl_vp8_lf_core.h states the rule, tests/vp8_lf_model.py restates it): the same again, but the frame header's loop filter
// level is the one of four candidates whose filtered reconstruction is nearest to the source; what a decoder shows is that filtered picture.
//
// seg: segment-adaptive quantisers (FLGPU_FEO_SEGMENTS, a bit of flgpu_params::options on any of the front ends; fl_vp8_seg_core.h
// states the rule, tests/vp8_seg_model.py restates it): the macroblocks are sorted into up to four classes by luma activity and
// each class is coded at a quantiser index of its own around the picture's; the frame header carries the segment header (absolute
// values, the frame's filter level in every segment) and every macroblock its id in front of its skip flag.  Where the rule finds
// nothing to separate, the stream is the one above ("one segment"), byte for byte.
#pragma once
#include <stdint.h>

#include "fl_vp8_dtables.h"
#include "fl_vp8_tables.h"

#if defined(__HIPCC__)
#define FL_VP8_HD __host__ __device__ inline
#else
#define FL_VP8_HD inline
#endif

namespace fl {

enum { VP8_DC = 0, VP8_V = 1, VP8_H = 2, VP8_TM = 3 };

constexpr uint32_t kVp8MaxSide = 16383;     // the frame header holds 14 bits of width and of height
constexpr uint32_t kVp8MbLevels = 25 * 16;  // levels of one macroblock in coding order: 16 Y, 4 U, 4 V blocks, then Y2
constexpr uint32_t kVp8I4PenaltyShift = 9;  // vp8_i4_penalty
constexpr int kVp8MaxLevel = 2047;          // the largest magnitude cat6 (67 + 11 bits) is asked to carry here

// ---- worst cases ----------------------------------------------------------------------------------------------------------------
// One rule for every variant (i4: macroblocks may be B_PRED; ap: per-picture probabilities; seg: FLGPU_FEO_SEGMENTS; the loop filter
// adds nothing, its level's six literals are header bits below): a boolean costs at most 7 bits -- the range is 128..255 before it
// and at least 1 after it, so renormalising shifts at most 7 --, and no size field of the format may overflow on the worst case.
// Partition 0 holds 29 header bits, 1056 "no update" flags, the skip switch and its probability (1 + 8), per macroblock the skip
// flag, 3 luma-mode and 3 chroma-mode booleans, and the 32 booleans of the flush: 1126 + 7 per macroblock.
// A coefficient costs at most 7 tree booleans + 11 extra bits + the sign = 19; a macroblock has 16 (Y2) + 16 x 15 (Y) + 8 x 16
// (U, V) = 384 of them (a block that is full has no end-of-block).  Each token partition adds the 32 booleans of its flush.
constexpr uint64_t kVp8BoolBits = 7;
constexpr uint64_t kVp8Part0Bools = 29 + 1056 + 9 + 32, kVp8Part0MbBools = 7;
constexpr uint64_t kVp8MbTokenBools = 384 * 19;
constexpr uint64_t kVp8FlushBools = 32;
// i4: a B_PRED macroblock has the skip flag, one luma-tree boolean, sixteen sub-block modes of at most 7 tree booleans (B_HD, B_HU:
// nodes 0, 1, 2, 3, 6, 7, 8) and 3 chroma-mode booleans: 1 + 1 + 16 x 7 + 3 = 117, against an I16 macroblock's 7.  Its tokens do
// not grow: 24 blocks x 16 coefficients = 384, what 16 (Y2) + 16 x 15 + 8 x 16 comes to.
constexpr uint64_t kVp8Part0MbBoolsI4 = 1 + 1 + 16 * 7 + 3;
// ap: each of the 1056 flags may be followed by an 8-bit probability.
constexpr uint64_t kVp8Part0BoolsAp = 29 + 1056 * 9 + 9 + 32; // 9574
// seg (fl_vp8_seg_core.h): partition 0 also holds the segment header -- update_mb_segmentation_map, update_segment_feature_data and
// segment_feature_mode (3), four quantisers of flag + 7 bits + sign (36), four filter strengths of flag + 6 bits + sign (32), three
// tree probabilities of flag + 8 bits (27): 98 -- and two booleans of segment id per macroblock.
constexpr uint64_t kVp8Part0SegBools = 3 + 4 * 9 + 4 * 8 + 3 * 9, kVp8Part0MbSegBools = 2;
static_assert(kVp8Part0SegBools == 98, "the segment header");

FL_VP8_HD constexpr uint64_t vp8_part0_fixed_bools(bool ap, bool seg) { return (ap ? kVp8Part0BoolsAp : kVp8Part0Bools) + (seg ? kVp8Part0SegBools : 0u); }
FL_VP8_HD constexpr uint64_t vp8_part0_mb_bools(bool i4, bool seg) { return (i4 ? kVp8Part0MbBoolsI4 : kVp8Part0MbBools) + (seg ? kVp8Part0MbSegBools : 0u); }
FL_VP8_HD constexpr uint64_t vp8_part0_max_bytes(uint64_t mbs, bool i4 = false, bool ap = false, bool seg = false)
{
    return (kVp8BoolBits * (vp8_part0_fixed_bools(ap, seg) + vp8_part0_mb_bools(i4, seg) * mbs) + 7u) / 8u;
}
// the first partition's size is a 19-bit field of the frame tag: the largest macroblock count whose worst case still fits it
FL_VP8_HD constexpr uint64_t vp8_max_mbs(bool i4 = false, bool ap = false, bool seg = false)
{
    return (((1ull << 19) - 1u) * 8u / kVp8BoolBits - vp8_part0_fixed_bools(ap, seg)) / vp8_part0_mb_bools(i4, seg);
}
constexpr bool vp8_part0_fits_its_field()
{
    for (int v = 0; v < 8; ++v) {
        const bool i4 = (v & 1) != 0, ap = (v & 2) != 0, seg = (v & 4) != 0;
        if (vp8_part0_max_bytes(vp8_max_mbs(i4, ap, seg), i4, ap, seg) >= (1ull << 19)) return false;
    }
    return true;
}
static_assert(vp8_part0_fits_its_field(), "first partition size field, every (i4, ap, seg)");
// the known values: B_PRED alone; with updates 72 macroblocks fewer; with segments 87 and 86 fewer than without
static_assert(vp8_max_mbs(true) == 5111 && vp8_max_mbs(true, true) == 5039 && vp8_max_mbs(true, false, true) == 5024 && vp8_max_mbs(true, true, true) == 4953, "the B_PRED variants' limits");
// (the 1056 literals are whole bytes of worst case: the partition-0 term grows by exactly 7 x 8448 / 8 = 7392)
static_assert(kVp8BoolBits * (kVp8Part0BoolsAp - kVp8Part0Bools) % 8u == 0 && vp8_part0_max_bytes(0, false, true) - vp8_part0_max_bytes(0) == 7392, "the updates' worst case");

FL_VP8_HD uint32_t vp8_mbs(uint32_t px) { return (px + 15u) >> 4; }
// token partitions: the largest of 1 / 2 / 4 / 8 that is not above the number of macroblock rows; row r goes to partition r mod n
FL_VP8_HD uint32_t vp8_partitions(uint32_t mb_rows) { return mb_rows >= 8 ? 8u : mb_rows >= 4 ? 4u : mb_rows >= 2 ? 2u : 1u; }
// a token partition's size is a 24-bit field: the worst case of the partition with the most rows
FL_VP8_HD uint64_t vp8_token_partition_max_bytes(uint64_t mbw, uint64_t mbh)
{
    const uint64_t np = vp8_partitions((uint32_t)mbh), rows = (mbh + np - 1u) / np;
    return (kVp8BoolBits * (kVp8MbTokenBools * rows * mbw + kVp8FlushBools) + 7u) / 8u;
}
// The pictures a variant takes: sides of at most 14 bits, and no size field that its worst case could overflow.  (Without B_PRED
// the 24-bit token partition field binds first, at about 21 000 macroblocks; with it, vp8_max_mbs.)  A picture that fits its front
// end but not the same with seg is coded without the option.
FL_VP8_HD bool vp8_fits(uint64_t w, uint64_t h, bool i4 = false, bool ap = false, bool seg = false)
{
    if (w < 1u || h < 1u || w > kVp8MaxSide || h > kVp8MaxSide) return false;
    const uint64_t mbw = (w + 15u) >> 4, mbh = (h + 15u) >> 4;
    return mbw * mbh <= vp8_max_mbs(i4, ap, seg) && vp8_token_partition_max_bytes(mbw, mbh) < (1ull << 24);
}
// The file's worst case: RIFF header (12), VP8X chunk (18), ALPH chunk (8 + 1 + w h + pad), VP8 chunk header (8), frame header (10),
// partition 0, seven partition sizes (21), the token partitions, the pad byte.  (Under vp8_fits this stays far below 2^32.)
FL_VP8_HD uint64_t vp8_max_out_bytes(uint64_t w, uint64_t h, bool i4 = false, bool ap = false, bool seg = false)
{
    const uint64_t mbs = ((w + 15u) >> 4) * ((h + 15u) >> 4);
    return 12u + 18u + (8u + 1u + w * h + 1u) + 8u + 10u + 21u + vp8_part0_max_bytes(mbs, i4, ap, seg) +
           (kVp8BoolBits * (kVp8MbTokenBools * mbs + 8u * kVp8FlushBools) + 7u) / 8u + 1u;
}

// ---- quantiser --------------------------------------------------------------------------------------------------------------------
struct Vp8Quant { uint16_t y1_dc, y1_ac, y2_dc, y2_ac, uv_dc, uv_ac; };

FL_VP8_HD uint32_t vp8_quality_index(uint32_t quality) { return kVp8QualityToIndex[quality > 100u ? 100u : quality]; }

FL_VP8_HD Vp8Quant vp8_quant(uint32_t qi)
{
    Vp8Quant q;
    q.y1_dc = kVp8DcStep[qi]; q.y1_ac = kVp8AcStep[qi];
    q.y2_dc = (uint16_t)(kVp8DcStep[qi] * 2u);
    const uint32_t y2ac = kVp8AcStep[qi] * 155u / 100u;
    q.y2_ac = (uint16_t)(y2ac < 8u ? 8u : y2ac);
    q.uv_dc = kVp8DcStep[qi > 117u ? 117u : qi]; // capped at 132
    q.uv_ac = kVp8AcStep[qi];
    return q;
}

// level of one coefficient: DC rounds to nearest, AC has a dead zone (bias 3/8 of a step); integer only
FL_VP8_HD int vp8_quantise(int c, int step, bool dc)
{
    const int a = c < 0 ? -c : c;
    int l = (a + (dc ? step >> 1 : (step * 3) >> 3)) / step;
    if (l > kVp8MaxLevel) l = kVp8MaxLevel;
    return c < 0 ? -l : l;
}

// The I4 variant's penalty on S4, from the y1_ac step: what the sixteen mode codes and the lost Y2 block are worth in squared error
// at that step (DESIGN.md holds the table it was tuned on).  Positive, so a macroblock whose I16 prediction is exact stays I16.
FL_VP8_HD uint32_t vp8_i4_penalty(uint32_t y1_ac)
{
    const uint64_t sq = (uint64_t)y1_ac * y1_ac, v = (sq * sq) >> kVp8I4PenaltyShift; // (steps are below 2^9: below 2^27)
    return v < 1u ? 1u : (uint32_t)v;
}

// ---- loop filter strength ---------------------------------------------------------------------------------------------------------
// The format's limits of a macroblock from its filter level (1..63) and the frame's sharpness: o[0] = the edge limit of inner edges
// (macroblock edges add 4), o[1] = the interior limit, o[2] = the high-edge-variance threshold of a key frame.  The decode front
// end's host half and the encoder's loop-filtered variants share it.
FL_VP8_HD void vp8_filter_strength(int level, int sharpness, uint8_t *o)
{
    int ilevel = level;
    if (sharpness > 0) {
        ilevel >>= sharpness > 4 ? 2 : 1;
        if (ilevel > 9 - sharpness) ilevel = 9 - sharpness;
    }
    if (ilevel < 1) ilevel = 1;
    o[0] = (uint8_t)(2 * level + ilevel); o[1] = (uint8_t)ilevel; o[2] = (uint8_t)(level >= 40 ? 2 : level >= 15 ? 1 : 0);
}

// ---- transforms -------------------------------------------------------------------------------------------------------------------
FL_VP8_HD int vp8_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// forward DCT of a 4x4 residual d (raster) -> out (raster); the encoder's own
// (its two passes apart, row i and column i: the I4 trial gives each to a lane)
FL_VP8_HD void vp8_fdct_row(const int *d, int *t, int i)
{
    const int a0 = d[4 * i] + d[4 * i + 3], a1 = d[4 * i + 1] + d[4 * i + 2], a2 = d[4 * i + 1] - d[4 * i + 2], a3 = d[4 * i] - d[4 * i + 3];
    t[4 * i] = (a0 + a1) * 8;
    t[4 * i + 1] = (a2 * 2217 + a3 * 5352 + 1812) >> 9;
    t[4 * i + 2] = (a0 - a1) * 8;
    t[4 * i + 3] = (a3 * 2217 - a2 * 5352 + 937) >> 9;
}
FL_VP8_HD void vp8_fdct_col(const int *t, int *out, int i)
{
    const int a0 = t[i] + t[12 + i], a1 = t[4 + i] + t[8 + i], a2 = t[4 + i] - t[8 + i], a3 = t[i] - t[12 + i];
    out[i] = (a0 + a1 + 7) >> 4;
    out[4 + i] = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0);
    out[8 + i] = (a0 - a1 + 7) >> 4;
    out[12 + i] = (a3 * 2217 - a2 * 5352 + 51000) >> 16;
}
FL_VP8_HD void vp8_fdct(const int *d, int *out)
{
    int t[16];
    for (int i = 0; i < 4; ++i) vp8_fdct_row(d, t, i);
    for (int i = 0; i < 4; ++i) vp8_fdct_col(t, out, i);
}

// forward Walsh-Hadamard transform of the 16 luma DCs (raster over the blocks); the encoder's own
FL_VP8_HD void vp8_fwht(const int *in, int *out)
{
    int t[16];
    for (int i = 0; i < 4; ++i) {
        const int a0 = in[4 * i] + in[4 * i + 2], a1 = in[4 * i + 1] + in[4 * i + 3], a2 = in[4 * i + 1] - in[4 * i + 3], a3 = in[4 * i] - in[4 * i + 2];
        t[4 * i] = a0 + a1; t[4 * i + 1] = a3 + a2; t[4 * i + 2] = a3 - a2; t[4 * i + 3] = a0 - a1;
    }
    for (int i = 0; i < 4; ++i) {
        const int a0 = t[i] + t[8 + i], a1 = t[4 + i] + t[12 + i], a2 = t[4 + i] - t[12 + i], a3 = t[i] - t[8 + i];
        out[i] = (a0 + a1) >> 1; out[4 + i] = (a3 + a2) >> 1; out[8 + i] = (a3 - a2) >> 1; out[12 + i] = (a0 - a1) >> 1;
    }
}

// the format's inverse WHT: dequantised Y2 coefficients (raster) -> the DC of each luma block (raster over the blocks)
FL_VP8_HD void vp8_iwht(const int *in, int *dc)
{
    int t[16];
    for (int i = 0; i < 4; ++i) {
        const int a0 = in[i] + in[12 + i], a1 = in[4 + i] + in[8 + i], a2 = in[4 + i] - in[8 + i], a3 = in[i] - in[12 + i];
        t[i] = a0 + a1; t[8 + i] = a0 - a1; t[4 + i] = a3 + a2; t[12 + i] = a3 - a2;
    }
    for (int i = 0; i < 4; ++i) {
        const int d = t[4 * i] + 3, a0 = d + t[4 * i + 3], a1 = t[4 * i + 1] + t[4 * i + 2], a2 = t[4 * i + 1] - t[4 * i + 2], a3 = d - t[4 * i + 3];
        dc[4 * i] = (a0 + a1) >> 3; dc[4 * i + 1] = (a3 + a2) >> 3; dc[4 * i + 2] = (a0 - a1) >> 3; dc[4 * i + 3] = (a3 - a2) >> 3;
    }
}

FL_VP8_HD int vp8_mul1(int a) { return ((a * 20091) >> 16) + a; }
FL_VP8_HD int vp8_mul2(int a) { return (a * 35468) >> 16; }

// the format's inverse DCT: dequantised coefficients (raster) -> the residual to add to the prediction (raster), before clamping
FL_VP8_HD void vp8_idct_col(const int *in, int *t, int i) // vertical pass, column i
{
    const int a = in[i] + in[8 + i], b = in[i] - in[8 + i];
    const int c = vp8_mul2(in[4 + i]) - vp8_mul1(in[12 + i]), d = vp8_mul1(in[4 + i]) + vp8_mul2(in[12 + i]);
    t[4 * i] = a + d; t[4 * i + 1] = b + c; t[4 * i + 2] = b - c; t[4 * i + 3] = a - d;
}
FL_VP8_HD void vp8_idct_row(const int *t, int *res, int i) // horizontal pass, row i
{
    const int dc = t[i] + 4, a = dc + t[8 + i], b = dc - t[8 + i];
    const int c = vp8_mul2(t[4 + i]) - vp8_mul1(t[12 + i]), d = vp8_mul1(t[4 + i]) + vp8_mul2(t[12 + i]);
    res[4 * i] = (a + d) >> 3; res[4 * i + 1] = (b + c) >> 3; res[4 * i + 2] = (b - c) >> 3; res[4 * i + 3] = (a - d) >> 3;
}
FL_VP8_HD void vp8_idct(const int *in, int *res)
{
    int t[16];
    for (int i = 0; i < 4; ++i) vp8_idct_col(in, t, i);
    for (int i = 0; i < 4; ++i) vp8_idct_row(t, res, i);
}

// ---- one picture ------------------------------------------------------------------------------------------------------------------
// What every phase needs to know about the picture.  src: the planes of FLGPU_FE_WEBP420 (Y | U | V | A, unpadded).  rec: the
// reconstruction, planes padded to whole macroblocks (Y 16 mbw x 16 mbh, then U and V 8 mbw x 8 mbh each).  lev: kVp8MbLevels
// levels per macroblock in coding order.  info: per macroblock, luma mode | chroma mode << 2 | non-zero flags << 4 (bit k of the
// flags: block k in the order of lev; a macroblock whose flags are all 0 is skipped).  bm (the I4 variant only): two words per
// macroblock, sixteen nibbles, sub-block b in nibble b & 7 of word b >> 3: the sub-block's mode (fl_vp8_dtables.h's numbers) in a
// B_PRED macroblock, 12 + the mode an I16 macroblock stands for in a neighbour's context otherwise.  A B_PRED macroblock has no
// Y2 block; bits 24 and 25 of its flags carry the Y2 context it passes on untouched, of its row (what the macroblock to its left
// has in bit 24) and of its column (what the one above passes on), and do not count towards "skipped".
struct Vp8Pic {
    const uint8_t *src;
    uint8_t *rec;
    int16_t *lev;
    uint32_t *info;
    uint32_t *bm = nullptr;
    const uint8_t *prob;   // kVp8CoefProb or, in the adaptive-probability variants, the picture's table; the kernels keep a copy in LDS
    uint32_t w, h, cw, ch, mbw, mbh;
    Vp8Quant q;            // the picture's steps; with FLGPU_FEO_SEGMENTS the current macroblock's (vp8_seg_pick)
    const struct Vp8SegRec *seg = nullptr; // FLGPU_FEO_SEGMENTS only: the picture's record and, per macroblock, its class
    const uint8_t *segmap = nullptr;
};

// What the segment rule (fl_vp8_seg_core.h) leaves of a picture: the quantiser index of each class, the probabilities of the
// segment tree, and whether the file is segmented at all (else the four indices are the picture's and every macroblock is class 0).
struct Vp8SegRec { uint8_t qi[4], prob[3], on; };
static_assert(sizeof(Vp8SegRec) == 8, "the record in scratch");
constexpr uint32_t kVp8SegHead = 16; // bytes of scratch in front of the class map
FL_VP8_HD uint64_t vp8_seg_bytes(uint64_t mbs) { return (kVp8SegHead + mbs + 15u) & ~(uint64_t)15u; }
// the steps of macroblock mb
FL_VP8_HD Vp8Quant vp8_mb_quant(const Vp8Pic &p, uint64_t mb) { return p.seg ? vp8_quant(p.seg->qi[p.segmap[mb] & 3u]) : p.q; }
// before the phases of macroblock mb: its class's steps become p.q (one branch, uniform over the picture)
FL_VP8_HD void vp8_seg_pick(Vp8Pic &p, uint64_t mb) { if (p.seg) p.q = vp8_quant(p.seg->qi[p.segmap[mb] & 3u]); }

FL_VP8_HD void vp8_pic_dims(Vp8Pic &p, uint32_t w, uint32_t h)
{
    p.prob = kVp8CoefProb;
    p.w = w; p.h = h; p.cw = (w + 1u) >> 1; p.ch = (h + 1u) >> 1; p.mbw = vp8_mbs(w); p.mbh = vp8_mbs(h);
}
FL_VP8_HD uint64_t vp8_rec_bytes(uint32_t mbw, uint32_t mbh) { return (uint64_t)mbw * mbh * 384u; }

// One macroblock's working set: LDS on the device, the stack on the host.  Planes are numbered 0 = Y, 1 = U, 2 = V; blocks 0..15
// are luma (raster), 16..19 U, 20..23 V.
struct Vp8Mb {
    uint8_t src[384];        // Y 16x16 at 0, U 8x8 at 256, V 8x8 at 320; source samples past the picture repeat its last row / column
    uint8_t top[3][20];      // [plane][0] = the top-left neighbour, [1..n] = the row above
    uint8_t left[3][16];
    int32_t dcv[3];          // the DC prediction's value per plane
    uint32_t sse_y[64], sse_uv[32];
    int32_t coef[24][16];    // forward DCT, raster
    int32_t ydc[16];         // reconstructed DC of the luma blocks (inverse WHT)
    int16_t lev[kVp8MbLevels];
    uint8_t nz[25];
    uint8_t ymode, uvmode;
};

// geometry of block b: plane, size of the plane's macroblock square, origin inside it, offset of the plane in Vp8Mb::src
FL_VP8_HD void vp8_block_geom(int b, int &plane, int &n, int &bx, int &by, int &off)
{
    if (b < 16) { plane = 0; n = 16; bx = (b & 3) * 4; by = (b >> 2) * 4; off = 0; }
    else { plane = 1 + ((b - 16) >> 2); n = 8; bx = (b & 1) * 4; by = ((b >> 1) & 1) * 4; off = plane == 1 ? 256 : 320; }
}

// the predicted sample at (x, y) of a plane's macroblock square
FL_VP8_HD int vp8_predict(const Vp8Mb &m, int plane, int mode, int x, int y)
{
    switch (mode) {
    case VP8_DC: return m.dcv[plane];
    case VP8_V: return m.top[plane][1 + x];
    case VP8_H: return m.left[plane][y];
    default: return vp8_clip8((int)m.top[plane][1 + x] + (int)m.left[plane][y] - (int)m.top[plane][0]);
    }
}

// Phase A, item k of 384 + 3 * 37: the source samples of the macroblock and its neighbours in the reconstruction.  Outside the
// frame the row above reads 127 and the column to the left 129; the top-left neighbour is 127 in the first row, else 129 in the
// first column (what the decoder's border initialisation amounts to).
FL_VP8_HD void vp8_phase_load(const Vp8Pic &p, Vp8Mb &m, uint32_t mbx, uint32_t mby, uint32_t k)
{
    const uint64_t ysz = (uint64_t)p.w * p.h, csz = (uint64_t)p.cw * p.ch;
    const uint64_t rys = (uint64_t)p.mbw * 16u, rcs = (uint64_t)p.mbw * 8u, rysz = rys * p.mbh * 16u, rcsz = rcs * p.mbh * 8u;
    if (k < 384u) {
        if (k < 256u) {
            uint32_t x = mbx * 16u + (k & 15u), y = mby * 16u + (k >> 4);
            x = x < p.w ? x : p.w - 1u; y = y < p.h ? y : p.h - 1u;
            m.src[k] = p.src[(uint64_t)y * p.w + x];
        } else {
            const uint32_t pl = (k - 256u) >> 6, i = (k - 256u) & 63u;
            uint32_t x = mbx * 8u + (i & 7u), y = mby * 8u + (i >> 3);
            x = x < p.cw ? x : p.cw - 1u; y = y < p.ch ? y : p.ch - 1u;
            m.src[k] = p.src[ysz + pl * csz + (uint64_t)y * p.cw + x];
        }
        return;
    }
    k -= 384u;
    const uint32_t plane = k / 37u, i = k % 37u, n = plane ? 8u : 16u;
    const uint8_t *r = plane == 0 ? p.rec : p.rec + rysz + (plane - 1u) * rcsz;
    const uint64_t rs = plane ? rcs : rys;
    const uint64_t x0 = (uint64_t)mbx * n, y0 = (uint64_t)mby * n;
    if (i == 0u) m.top[plane][0] = mby == 0u ? 127 : mbx == 0u ? 129 : r[(y0 - 1u) * rs + x0 - 1u];
    else if (i <= 16u) { if (i <= n) m.top[plane][i] = mby == 0u ? 127 : r[(y0 - 1u) * rs + x0 + i - 1u]; }
    else if (i - 17u < n) m.left[plane][i - 17u] = mbx == 0u ? 129 : r[(y0 + i - 17u) * rs + x0 - 1u];
}
constexpr uint32_t kVp8LoadItems = 384 + 3 * 37;

// Phase B, item = plane: the value of the DC prediction
FL_VP8_HD void vp8_phase_dc(Vp8Mb &m, uint32_t mbx, uint32_t mby, uint32_t plane)
{
    const int n = plane ? 8 : 16, sh = plane ? 3 : 4;
    int st = 0, sl = 0;
    for (int i = 0; i < n; ++i) { st += m.top[plane][1 + i]; sl += m.left[plane][i]; }
    if (mby && mbx) m.dcv[plane] = (st + sl + n) >> (sh + 1);
    else if (mby) m.dcv[plane] = (st + (n >> 1)) >> sh;
    else if (mbx) m.dcv[plane] = (sl + (n >> 1)) >> sh;
    else m.dcv[plane] = 128;
}

FL_VP8_HD uint32_t vp8_block_sse(const Vp8Mb &m, int b, int mode)
{
    int plane, n, bx, by, off;
    vp8_block_geom(b, plane, n, bx, by, off);
    uint32_t s = 0;
    for (int y = by; y < by + 4; ++y)
        for (int x = bx; x < bx + 4; ++x) {
            const int d = (int)m.src[off + y * n + x] - vp8_predict(m, plane, mode, x, y);
            s += (uint32_t)(d * d);
        }
    return s;
}
// Phase C, item k of 96: the SSE of one mode on one 4x4 block.  k < 64: luma, mode k / 16, block k % 16; else chroma, mode
// (k - 64) / 8, block 16 + (k - 64) % 8.
FL_VP8_HD void vp8_phase_sse(Vp8Mb &m, uint32_t k)
{
    if (k < 64u) m.sse_y[k] = vp8_block_sse(m, (int)(k & 15u), (int)(k >> 4));
    else m.sse_uv[k - 64u] = vp8_block_sse(m, 16 + (int)((k - 64u) & 7u), (int)((k - 64u) >> 3));
}
constexpr uint32_t kVp8SseItems = 96;

// Phase D (one item): the modes.  A later mode replaces an earlier one only if it is strictly better.
FL_VP8_HD void vp8_phase_modes(Vp8Mb &m)
{
    uint32_t best = 0xffffffffu;
    for (int mode = 0; mode < 4; ++mode) {
        uint32_t s = 0;
        for (int b = 0; b < 16; ++b) s += m.sse_y[mode * 16 + b];
        if (s < best) { best = s; m.ymode = (uint8_t)mode; }
    }
    best = 0xffffffffu;
    for (int mode = 0; mode < 4; ++mode) {
        uint32_t s = 0;
        for (int b = 0; b < 8; ++b) s += m.sse_uv[mode * 8 + b];
        if (s < best) { best = s; m.uvmode = (uint8_t)mode; }
    }
}

// Phase E, item = block b of 24: residual and forward DCT
FL_VP8_HD void vp8_phase_fdct(Vp8Mb &m, uint32_t b)
{
    int plane, n, bx, by, off, d[16], o[16];
    vp8_block_geom((int)b, plane, n, bx, by, off);
    const int mode = plane ? m.uvmode : m.ymode;
    for (int y = 0; y < 4; ++y)
        for (int x = 0; x < 4; ++x) d[4 * y + x] = (int)m.src[off + (by + y) * n + bx + x] - vp8_predict(m, plane, mode, bx + x, by + y);
    vp8_fdct(d, o);
    for (int i = 0; i < 16; ++i) m.coef[b][i] = o[i];
}

// Phase F (one item): the luma DCs through the WHT, its levels (block 24) and the DCs the decoder will see
FL_VP8_HD void vp8_phase_y2(const Vp8Pic &p, Vp8Mb &m)
{
    int in[16], w[16], dq[16], dc[16];
    for (int b = 0; b < 16; ++b) in[b] = m.coef[b][0];
    vp8_fwht(in, w);
    int any = 0;
    for (int i = 0; i < 16; ++i) dq[i] = 0;
    for (int n = 0; n < 16; ++n) {
        const int r = kVp8Zigzag[n], step = n ? p.q.y2_ac : p.q.y2_dc;
        const int l = vp8_quantise(w[r], step, n == 0);
        m.lev[24 * 16 + n] = (int16_t)l;
        dq[r] = l * step;
        any |= l;
    }
    m.nz[24] = any != 0;
    vp8_iwht(dq, dc);
    for (int b = 0; b < 16; ++b) m.ydc[b] = dc[b];
}

// Phase G, item = block b of 24: levels, and the reconstruction the decoder will compute, written to the picture's planes
FL_VP8_HD void vp8_phase_recon(const Vp8Pic &p, Vp8Mb &m, uint32_t mbx, uint32_t mby, uint32_t b)
{
    int plane, n, bx, by, off, dq[16], res[16];
    vp8_block_geom((int)b, plane, n, bx, by, off);
    const int mode = plane ? m.uvmode : m.ymode;
    const int dcs = plane ? p.q.uv_dc : p.q.y1_dc, acs = plane ? p.q.uv_ac : p.q.y1_ac;
    int any = 0;
    for (int i = 0; i < 16; ++i) dq[i] = 0;
    for (int k = 0; k < 16; ++k) {
        const int r = kVp8Zigzag[k];
        int l = 0;
        if (k || plane) l = vp8_quantise(m.coef[b][r], k ? acs : dcs, k == 0);
        m.lev[b * 16 + k] = (int16_t)l;
        dq[r] = l * (k ? acs : dcs);
        any |= l;
    }
    m.nz[b] = any != 0;
    if (!plane) dq[0] = m.ydc[b];
    vp8_idct(dq, res);
    const uint64_t rys = (uint64_t)p.mbw * 16u, rcs = (uint64_t)p.mbw * 8u, rysz = rys * p.mbh * 16u, rcsz = rcs * p.mbh * 8u;
    uint8_t *r = plane == 0 ? p.rec : p.rec + rysz + (uint64_t)(plane - 1) * rcsz;
    const uint64_t rs = plane ? rcs : rys;
    for (int y = 0; y < 4; ++y)
        for (int x = 0; x < 4; ++x)
            r[((uint64_t)mby * n + by + y) * rs + (uint64_t)mbx * n + bx + x] = (uint8_t)vp8_clip8(vp8_predict(m, plane, mode, bx + x, by + y) + res[4 * y + x]);
}

// Phase H, item k of kVp8MbLevels + 1: the macroblock's levels and its record go to the picture's arrays
FL_VP8_HD void vp8_phase_store(const Vp8Pic &p, const Vp8Mb &m, uint32_t mbx, uint32_t mby, uint32_t k)
{
    const uint64_t mb = (uint64_t)mby * p.mbw + mbx;
    if (k < kVp8MbLevels) { p.lev[mb * kVp8MbLevels + k] = m.lev[k]; return; }
    uint32_t nz = 0;
    for (int b = 0; b < 25; ++b) nz |= (uint32_t)m.nz[b] << b;
    p.info[mb] = (uint32_t)m.ymode | (uint32_t)m.uvmode << 2 | nz << 4;
}

// ---- boolean coder ----------------------------------------------------------------------------------------------------------------
// The arithmetic coder of section 7 in its usual carry-propagating form.  buf == nullptr only counts: the same states, no stores.
struct Vp8Bool {
    uint32_t low = 0, range = 255, pos = 0;
    int count = -24;
    uint8_t *buf = nullptr;

    FL_VP8_HD void put(int bit, uint32_t prob)
    {
        const uint32_t split = 1u + (((range - 1u) * prob) >> 8);
        if (bit) { low += split; range -= split; } else range = split;
        int shift = __builtin_clz(range) - 24;
        range <<= shift;
        count += shift;
        if (count >= 0) {
            const int offset = shift - count;
            if (buf) {
                if ((low << (offset - 1)) & 0x80000000u) { // carry into the bytes already written
                    uint32_t x = pos;
                    while (x > 0u && buf[x - 1u] == 0xffu) { buf[x - 1u] = 0; --x; }
                    if (x > 0u) buf[x - 1u] = (uint8_t)(buf[x - 1u] + 1u);
                }
                buf[pos] = (uint8_t)(low >> (24 - offset));
            }
            ++pos;
            low = (low << offset) & 0xffffffu;
            shift = count;
            count -= 8;
        }
        low <<= shift;
    }
    // the sink of the token walk (vp8_put_block): a boolean whose probability is an entry of the coefficient table, here just coded
    FL_VP8_HD void node(int bit, const uint8_t *p) { put(bit, *p); }
    FL_VP8_HD void literal(uint32_t v, int bits) { for (int b = bits - 1; b >= 0; --b) put((int)((v >> b) & 1u), 128u); }
    FL_VP8_HD void flush() { for (int i = 0; i < 32; ++i) put(0, 128u); }
};

// ---- partitions -------------------------------------------------------------------------------------------------------------------
FL_VP8_HD const uint8_t *vp8_prob(const uint8_t *tab, int type, int n, int ctx) { return tab + ((type * 8 + kVp8Band[n]) * 3 + ctx) * 11; }

// the tokens of one block: src = its 16 levels in coding order (32 bytes, 16-byte aligned: fetched whole, not one by one), from
// position `first`.  The one walk of the token tree: `bw` is a sink with node(bit, p) for a boolean whose probability is the entry p
// of the coefficient table and put(bit, prob) for any other (sign and extra bits) -- Vp8Bool codes both, Vp8Count
// (fl_vp8_ap_core.h) counts the first kind per entry and drops the second.
template <class Sink> FL_VP8_HD void vp8_put_block(Sink &bw, const uint8_t *tab, const int16_t *src, int type, int first, int ctx)
{
    int16_t lev[16];
    __builtin_memcpy(lev, __builtin_assume_aligned(src, 16), sizeof(lev));
    int last = -1;
    for (int i = first; i < 16; ++i) if (lev[i]) last = i;
    int n = first;
    const uint8_t *p = vp8_prob(tab, type, n, ctx);
    bw.node(last >= 0, p);
    if (last < 0) return;
    while (n < 16) {
        const int c = lev[n++];
        const int v = c < 0 ? -c : c;
        if (v == 0) { bw.node(0, p + 1); p = vp8_prob(tab, type, n, 0); continue; }
        bw.node(1, p + 1);
        if (v == 1) { bw.node(0, p + 2); p = vp8_prob(tab, type, n, 1); }
        else {
            bw.node(1, p + 2);
            if (v <= 4) {
                bw.node(0, p + 3);
                bw.node(v != 2, p + 4);
                if (v != 2) bw.node(v == 4, p + 5);
            } else {
                bw.node(1, p + 3);
                int cat;
                if (v <= 10) { bw.node(0, p + 6); cat = v > 6; bw.node(cat, p + 7); }
                else {
                    bw.node(1, p + 6);
                    cat = v < 19 ? 2 : v < 35 ? 3 : v < 67 ? 4 : 5;
                    bw.node(cat >= 4, p + 8);
                    bw.node(cat & 1, p + (cat >= 4 ? 10 : 9));
                }
                const int extra = v - (int)kVp8CatBase[cat];
                for (int k = (int)kVp8CatBits[cat] - 1, t = 0; k >= 0; --k, ++t) bw.put((extra >> k) & 1, kVp8CatProb[cat][t]);
            }
            p = vp8_prob(tab, type, n, 2);
        }
        bw.put(c < 0, 128u);
        if (n == 16) return;
        bw.node(n <= last, p);
        if (n > last) return;
    }
}

FL_VP8_HD uint32_t vp8_nz(const Vp8Pic &p, uint32_t mbx, uint32_t mby) { return p.info[(uint64_t)mby * p.mbw + mbx] >> 4; }

// ---- the I4 variant's records ---------------------------------------------------------------------------------------------------
constexpr uint32_t kVp8BmI16 = 12;            // nibble of an I16 macroblock's record: 12 + its context mode (0..3)
constexpr uint32_t kVp8NzBlocks = 0xffffffu;  // the 24 blocks a B_PRED macroblock codes
FL_VP8_HD uint32_t vp8_bm_nibble(const Vp8Pic &p, uint64_t mb, uint32_t b) { return (p.bm[2u * mb + (b >> 3)] >> (4u * (b & 7u))) & 15u; }
FL_VP8_HD bool vp8_is_i4(const Vp8Pic &p, uint64_t mb) { return (p.bm[2u * mb] & 15u) < kVp8BmI16; }
FL_VP8_HD uint32_t vp8_bm_context(uint32_t nibble) { return nibble < kVp8BmI16 ? nibble : nibble - kVp8BmI16; }
// the mode an I16 macroblock stands for in the context of a neighbouring sub-block
FL_VP8_HD uint32_t vp8_context_mode(uint32_t ymode) { return ymode == VP8_DC ? VP8_B_DC : ymode == VP8_V ? VP8_B_VE : ymode == VP8_H ? VP8_B_HE : VP8_B_TM; }
// the flags that decide whether a macroblock is skipped
template <bool I4> FL_VP8_HD uint32_t vp8_coded(const Vp8Pic &p, uint64_t mb)
{
    const uint32_t nz = p.info[mb] >> 4;
    if (I4) return vp8_is_i4(p, mb) ? nz & kVp8NzBlocks : nz;
    return nz;
}

// one sub-block mode through the tree of section 11.2 (fl_vp8_dtables.h draws it); pr: the nine probabilities of its context
FL_VP8_HD void vp8_put_bmode(Vp8Bool &bw, uint32_t m, const uint8_t *pr)
{
    bw.put(m != VP8_B_DC, pr[0]);
    if (m == VP8_B_DC) return;
    bw.put(m != VP8_B_TM, pr[1]);
    if (m == VP8_B_TM) return;
    bw.put(m != VP8_B_VE, pr[2]);
    if (m == VP8_B_VE) return;
    const bool far = m == VP8_B_LD || m >= VP8_B_VL;
    bw.put(far, pr[3]);
    if (!far) {
        bw.put(m != VP8_B_HE, pr[4]);
        if (m != VP8_B_HE) bw.put(m == VP8_B_VR, pr[5]);
        return;
    }
    bw.put(m != VP8_B_LD, pr[6]);
    if (m == VP8_B_LD) return;
    bw.put(m != VP8_B_VL, pr[7]);
    if (m != VP8_B_VL) bw.put(m == VP8_B_HU, pr[8]);
}

// the sixteen modes of B_PRED macroblock (mbx, mby), each in the context of the modes above it and to its left
FL_VP8_HD void vp8_put_bmodes(Vp8Bool &bw, const Vp8Pic &p, uint32_t mbx, uint32_t mby)
{
    const uint64_t mb = (uint64_t)mby * p.mbw + mbx;
    for (uint32_t b = 0; b < 16u; ++b) {
        const uint32_t above = (b >> 2) ? vp8_bm_nibble(p, mb, b - 4u) : mby ? vp8_bm_context(vp8_bm_nibble(p, mb - p.mbw, b + 12u)) : (uint32_t)VP8_B_DC;
        const uint32_t left = (b & 3u) ? vp8_bm_nibble(p, mb, b - 1u) : mbx ? vp8_bm_context(vp8_bm_nibble(p, mb - 1u, b + 3u)) : (uint32_t)VP8_B_DC;
        vp8_put_bmode(bw, vp8_bm_nibble(p, mb, b), kVp8BModeProb + (above * 10u + left) * 9u);
    }
}

// What the blocks of one macroblock are coded with: its own non-zero flags, those of the macroblocks to the left and above (0
// outside the frame), the Y2 context from above, whether it is B_PRED, its levels.  coded == 0: it is skipped.
struct Vp8MbCtx {
    uint32_t coded, nz, lnz, tnz, t24;
    bool i4;
    const int16_t *lev;
};
template <bool I4> FL_VP8_HD Vp8MbCtx vp8_mb_ctx(const Vp8Pic &p, uint32_t mbx, uint32_t mby)
{
    const uint64_t mb = (uint64_t)mby * p.mbw + mbx;
    Vp8MbCtx c;
    c.i4 = I4 && vp8_is_i4(p, mb);
    c.nz = vp8_nz(p, mbx, mby);
    c.coded = c.i4 ? c.nz & kVp8NzBlocks : c.nz;
    c.lnz = c.tnz = c.t24 = 0u;
    c.lev = p.lev + mb * kVp8MbLevels;
    if (!c.coded) return c;
    c.lnz = mbx ? vp8_nz(p, mbx - 1u, mby) : 0u;
    c.tnz = mby ? vp8_nz(p, mbx, mby - 1u) : 0u;
    if (!c.i4) c.t24 = I4 && mby && vp8_is_i4(p, mb - p.mbw) ? c.tnz >> 25 : c.tnz >> 24;
    return c;
}
// the tokens of block b of a coded macroblock, b in the order of lev: 0..15 luma, 16..23 chroma, 24 the Y2 block (an I16 macroblock's only)
template <class Sink> FL_VP8_HD void vp8_put_mb_block(Sink &bw, const uint8_t *tab, const Vp8MbCtx &c, uint32_t b)
{
    if (b == 24u) {
        if (!c.i4) vp8_put_block(bw, tab, c.lev + 24 * 16, 1, 0, (int)((c.lnz >> 24) & 1u) + (int)(c.t24 & 1u));
    } else if (b < 16u) {
        const uint32_t l = (b & 3u) ? c.nz >> (b - 1u) : c.lnz >> (b + 3u), t = (b >> 2) ? c.nz >> (b - 4u) : c.tnz >> (b + 12u);
        vp8_put_block(bw, tab, c.lev + b * 16, c.i4 ? 3 : 0, c.i4 ? 0 : 1, (int)(l & 1u) + (int)(t & 1u));
    } else {
        const uint32_t l = (b & 1u) ? c.nz >> (b - 1u) : c.lnz >> (b + 1u), t = (b & 2u) ? c.nz >> (b - 2u) : c.tnz >> (b + 2u);
        vp8_put_block(bw, tab, c.lev + b * 16, 2, 0, (int)(l & 1u) + (int)(t & 1u));
    }
}
constexpr uint32_t kVp8MbBlocks = 25;

// the tokens of one macroblock in the stream's order: Y2, luma, chroma
template <bool I4 = false, class Sink> FL_VP8_HD void vp8_put_mb(Sink &bw, const Vp8Pic &p, uint32_t mbx, uint32_t mby)
{
    const Vp8MbCtx c = vp8_mb_ctx<I4>(p, mbx, mby);
    if (!c.coded) return; // skipped
    vp8_put_mb_block(bw, p.prob, c, 24u);
    for (uint32_t b = 0; b < 16; ++b) vp8_put_mb_block(bw, p.prob, c, b);
    for (uint32_t b = 16; b < 24; ++b) vp8_put_mb_block(bw, p.prob, c, b);
}

// token partition `part` of `nparts`: the macroblock rows part, part + nparts, ...
// (always inlined: with four coder kernels per variant calling it, the compiler would otherwise keep it a function of its own,
// whose block buffer then lives in scratch memory instead of LDS)
template <bool I4 = false> __attribute__((always_inline)) FL_VP8_HD void vp8_put_token_partition(Vp8Bool &bw, const Vp8Pic &p, uint32_t part, uint32_t nparts)
{
    for (uint32_t mby = part; mby < p.mbh; mby += nparts)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) vp8_put_mb<I4>(bw, p, mbx, mby);
    bw.flush();
}

// probability that a macroblock is NOT skipped, from the picture's count of skipped ones: round(255 coded / all), at least 1
FL_VP8_HD uint32_t vp8_skip_prob(uint32_t mbs, uint32_t skipped)
{
    const uint32_t pr = ((mbs - skipped) * 255u + mbs / 2u) / mbs;
    return pr < 1u ? 1u : pr;
}

// partition 0: the frame header and every macroblock's skip flag and modes.  AP (the adaptive-probability variants): p.prob is the
// picture's table, and entry i is updated exactly where it differs from the default one (the rule never picks an equal value)
// LF (the loop-filtered variants, fl_vp8_lf_core.h): `level` is the loop filter level of the frame header; else it is 0
// p.seg (FLGPU_FEO_SEGMENTS, at run time): a segmented picture's header and, per macroblock, its id in front of the skip flag
template <bool I4 = false, bool AP = false, bool LF = false> FL_VP8_HD void vp8_put_first_partition(Vp8Bool &bw, const Vp8Pic &p, uint32_t qi, uint32_t nparts, uint32_t level = 0u)
{
    const uint32_t mbs = p.mbw * p.mbh;
    uint32_t skipped = 0;
    for (uint32_t mb = 0; mb < mbs; ++mb) skipped += vp8_coded<I4>(p, mb) == 0u;
    const uint32_t ps = vp8_skip_prob(mbs, skipped);
    bw.literal(0, 1);                       // colour space
    bw.literal(0, 1);                       // clamping is needed
    const bool seg = p.seg && p.seg->on;    // FLGPU_FEO_SEGMENTS and the rule found classes that differ
    bw.literal(seg, 1);                     // segmentation_enabled
    if (seg) {
        bw.literal(1, 1); bw.literal(1, 1); bw.literal(1, 1); // update the map, update the data, absolute values
        for (int k = 0; k < 4; ++k) { bw.literal(1, 1); bw.literal(p.seg->qi[k], 7); bw.literal(0, 1); }
        // (under absolute values a decoder takes a macroblock's filter level from its segment: the frame's, four times)
        for (int k = 0; k < 4; ++k) { bw.literal(LF && level, 1); if (LF && level) { bw.literal(level, 6); bw.literal(0, 1); } }
        for (int k = 0; k < 3; ++k) { bw.literal(p.seg->prob[k] != 255u, 1); if (p.seg->prob[k] != 255u) bw.literal(p.seg->prob[k], 8); }
    }
    bw.literal(0, 1); bw.literal(LF ? level : 0u, 6); bw.literal(0, 3); // normal filter, its level, sharpness 0
    bw.literal(0, 1);                       // no filter deltas
    bw.literal(nparts == 8u ? 3u : nparts == 4u ? 2u : nparts == 2u ? 1u : 0u, 2);
    bw.literal(qi, 7);
    for (int i = 0; i < 5; ++i) bw.literal(0, 1); // no quantiser deltas
    bw.literal(0, 1);                       // refresh_entropy_probs
    for (int i = 0; i < 4 * 8 * 3 * 11; ++i) {
        const bool update = AP && p.prob[i] != kVp8CoefProb[i];
        bw.put(update, kVp8CoefUpdateProb[i]);
        if (update) bw.literal(p.prob[i], 8);
    }
    bw.literal(1, 1);                       // mb_no_coeff_skip
    bw.literal(ps, 8);
    for (uint32_t mb = 0; mb < mbs; ++mb) {
        const uint32_t info = p.info[mb], ym = info & 3u, uvm = (info >> 2) & 3u;
        if (seg) {
            const uint32_t s = p.segmap[mb];
            bw.put(s >= 2u, p.seg->prob[0]);
            bw.put(s & 1u, s >= 2u ? p.seg->prob[2] : p.seg->prob[1]);
        }
        bw.put(vp8_coded<I4>(p, mb) == 0u, ps);
        if (I4 && vp8_is_i4(p, mb)) {
            bw.put(0, kVp8YModeProb[0]);
            vp8_put_bmodes(bw, p, mb % p.mbw, mb / p.mbw);
        } else {
            bw.put(1, kVp8YModeProb[0]);
            bw.put(ym >= 2u, kVp8YModeProb[1]);
            bw.put(ym & 1u, ym >= 2u ? kVp8YModeProb[3] : kVp8YModeProb[2]);
        }
        bw.put(uvm != 0u, kVp8UvModeProb[0]);
        if (uvm) { bw.put(uvm != 1u, kVp8UvModeProb[1]); if (uvm != 1u) bw.put(uvm == 3u, kVp8UvModeProb[2]); }
    }
    bw.flush();
}

// ---- the file -----------------------------------------------------------------------------------------------------------------------
// Offsets of the file's parts from the partitions' sizes (size[0] = partition 0, size[1 + k] = token partition k).
struct Vp8Layout {
    uint32_t alph;      // offset of the ALPH chunk header (0: none)
    uint32_t alph_size; // payload of the ALPH chunk: its header byte and the plane, raw (1 + w h) or as a VP8L stream (less)
    uint32_t vp8;       // offset of the "VP8 " chunk header
    uint32_t part[9];   // offset of every partition
    uint32_t vp8_size;  // payload of the VP8 chunk
    uint32_t total;     // file bytes
};

// The ALPH payload of a plane whose VP8L stream has `stream_bytes` bytes (0: there is none): the stream behind its header byte iff
// that is strictly smaller than the raw plane behind its, else the raw one.  A file is never larger than with the raw plane.
FL_VP8_HD uint32_t vp8_alph_size(uint32_t w, uint32_t h, uint32_t stream_bytes) { return stream_bytes && stream_bytes < w * h ? 1u + stream_bytes : 1u + w * h; }

// alph_size: vp8_alph_size of a translucent picture (0: the raw plane)
FL_VP8_HD Vp8Layout vp8_layout(uint32_t w, uint32_t h, bool alpha, uint32_t nparts, const uint32_t *size, uint32_t alph_size = 0u)
{
    Vp8Layout L;
    uint32_t o = 12u;
    L.alph = 0u;
    L.alph_size = alpha ? (alph_size ? alph_size : 1u + w * h) : 0u;
    if (alpha) { o += 18u; L.alph = o; o += 8u + L.alph_size; o += o & 1u; }
    L.vp8 = o;
    o += 8u + 10u;
    L.part[0] = o;                       // partition 0, then the sizes of all token partitions but the last, then those partitions
    o += size[0] + 3u * (nparts - 1u);
    for (uint32_t k = 1; k <= nparts; ++k) { L.part[k] = o; o += size[k]; }
    for (uint32_t k = nparts + 1u; k < 9u; ++k) L.part[k] = o;
    L.vp8_size = o - L.vp8 - 8u;
    L.total = o + (o & 1u);
    return L;
}

FL_VP8_HD void vp8_put_le(uint8_t *d, uint32_t v, int bytes) { for (int i = 0; i < bytes; ++i) d[i] = (uint8_t)(v >> (8 * i)); }
FL_VP8_HD void vp8_put_tag(uint8_t *d, const char *t) { for (int i = 0; i < 4; ++i) d[i] = (uint8_t)t[i]; }

// Everything of the file that is not a partition or the alpha plane's bytes: RIFF header, VP8X and ALPH headers where the picture
// is translucent (the ALPH header byte says raw, or lossless without filter or pre-processing, by the payload's size), the VP8 chunk
// header, frame tag, start code, dimensions, partition sizes, pad bytes.
FL_VP8_HD void vp8_put_framing(uint8_t *d, const Vp8Layout &L, uint32_t w, uint32_t h, bool alpha, uint32_t nparts, const uint32_t *size)
{
    vp8_put_tag(d, "RIFF"); vp8_put_le(d + 4, L.total - 8u, 4); vp8_put_tag(d + 8, "WEBP");
    if (alpha) {
        vp8_put_tag(d + 12, "VP8X"); vp8_put_le(d + 16, 10u, 4);
        vp8_put_le(d + 20, 0x10u, 4);                               // flags: alpha
        vp8_put_le(d + 24, w - 1u, 3); vp8_put_le(d + 27, h - 1u, 3);
        vp8_put_tag(d + L.alph, "ALPH"); vp8_put_le(d + L.alph + 4, L.alph_size, 4);
        d[L.alph + 8u] = L.alph_size != 1u + w * h ? 1 : 0;         // compression (VP8L or none), no filter, no pre-processing
        if (L.alph_size & 1u) d[L.vp8 - 1u] = 0;
    }
    uint8_t *f = d + L.vp8;
    vp8_put_tag(f, "VP8 "); vp8_put_le(f + 4, L.vp8_size, 4);
    vp8_put_le(f + 8, 0u | 0u << 1 | 1u << 4 | size[0] << 5, 3);    // key frame, version 0, shown, size of partition 0
    f[11] = 0x9d; f[12] = 0x01; f[13] = 0x2a;
    vp8_put_le(f + 14, w, 2); vp8_put_le(f + 16, h, 2);             // no scaling
    for (uint32_t k = 1; k < nparts; ++k) vp8_put_le(f + 18 + size[0] + 3 * (k - 1), size[k], 3);
    if (L.vp8_size & 1u) d[L.total - 1u] = 0;
}

} // namespace fl
