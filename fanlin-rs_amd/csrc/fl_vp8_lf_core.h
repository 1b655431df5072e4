// fl_vp8_lf_core.h -- the loop-filtered variants of the lossy WebP encoder (FLGPU_FE_WEBP_LOSSY_LF, _I4_LF, _AP_LF, _I4_AP_LF): the
// rule that picks the frame header's loop filter level, as code that compiles for the host and for the device.  Each variant codes
// the macroblocks, modes, levels and probabilities of the front end it stands beside; only the 6-bit level literal differs (and with
// it the bytes of partition 0).  tests/vp8_lf_model.py restates the rule, tests/vp8_host.cpp runs it in plain loops.
//
// The rule, integer only:
//   * base level from the quantiser index: s = min(y1_ac(qi) >> 2, 63), f = s * 300 / 256, L0 = 0 if f < 2 else min(f, 63).
//     (libwebp's SetupFilterStrength at filter_strength 60, sharpness 0, one segment, as recalled -- not pinned against libwebp.)
//   * candidates: 0, ceil(L0 / 2), L0, min(63, L0 + ceil(L0 / 2)).
//   * a candidate c > 0 is judged by doing what a decoder will do with it: the format's normal filter (section 15), sharpness 0,
//     no deltas, on a copy of the padded reconstruction; macroblocks in raster order, in each the left edge, the inner vertical
//     edges, the top edge, the inner horizontal edges (vp8d_filter of fl_vp8dec_core.h, the decode front end's); limits from c by
//     vp8_filter_strength, the derivation the decode front end uses.  Inner edges are filtered iff the macroblock is B_PRED or has
//     a coefficient left: a non-zero luma AC or chroma level, or a luma DC that the inverse WHT of the dequantised Y2 block leaves
//     non-zero (vp8_lf_inner) -- the decoder's rule, so a macroblock whose Y2 levels give sixteen zero DCs is coded, yet its inner
//     edges stay.
//   * D(c): the sum over Y, U, V of squared differences between the filtered copy and the source planes over the visible w x h
//     luma and ceil(w / 2) x ceil(h / 2) chroma samples (the padding is excluded), in 64 bits.  D(0) is the reconstruction's.
//   * the level written is the candidate with the least D; ties go to the lowest level (vp8_lf_choice).
//   * L0 = 0: nothing is evaluated, the four words are 0, and the file is the twin front end's byte for byte.
#pragma once
#include "fl_vp8_core.h"
#include "fl_vp8dec_core.h"

namespace fl {

constexpr uint32_t kVp8LfCandidates = 4;
constexpr uint32_t kVp8LfCostBytes = 256; // per picture, in front of its three copies: four 64-bit words, padded

FL_VP8_HD uint32_t vp8_lf_base(uint32_t qi)
{
    uint32_t s = kVp8AcStep[qi] >> 2;
    s = s > 63u ? 63u : s;
    const uint32_t f = s * 300u / 256u;
    return f < 2u ? 0u : f > 63u ? 63u : f;
}
// forced < 0: from the quantiser; else the debug hook's value
FL_VP8_HD uint32_t vp8_lf_base_of(uint32_t qi, int32_t forced) { return forced < 0 ? vp8_lf_base(qi) : forced > 63 ? 63u : (uint32_t)forced; }

FL_VP8_HD uint32_t vp8_lf_candidate(uint32_t base, uint32_t k)
{
    const uint32_t half = (base + 1u) >> 1, top = base + half;
    return k == 0u ? 0u : k == 1u ? half : k == 2u ? base : top > 63u ? 63u : top;
}

// the level of the frame header from the base level and the four cost words
FL_VP8_HD uint32_t vp8_lf_choice(uint32_t base, const uint64_t *D)
{
    if (base == 0u) return 0u;
    uint32_t best = 0u;
    for (uint32_t k = 1; k < kVp8LfCandidates; ++k)
        if (D[k] < D[best]) best = k; // (candidates ascend: the first of equal costs is the lowest level)
    return vp8_lf_candidate(base, best);
}

// does the decoder filter the inner edges of macroblock mb?
template <bool I4> FL_VP8_HD bool vp8_lf_inner(const Vp8Pic &p, uint64_t mb)
{
    if (I4 && vp8_is_i4(p, mb)) return true;
    const uint32_t nz = p.info[mb] >> 4;
    if (nz & kVp8NzBlocks) return true;
    if (!((nz >> 24) & 1u)) return false;
    // only Y2 levels: the luma DCs the decoder will see
    const int16_t *l = p.lev + mb * kVp8MbLevels + 24u * 16u;
    int in[16], dc[16];
    const Vp8Quant q = vp8_mb_quant(p, mb); // (with FLGPU_FEO_SEGMENTS: the steps a decoder takes for this macroblock's segment)
    for (int k = 0; k < 16; ++k) in[kVp8Zigzag[k]] = (int16_t)(l[k] * (int)(k ? q.y2_ac : q.y2_dc));
    vp8_iwht(in, dc);
    bool any = false;
    for (int b = 0; b < 16; ++b) any |= (int16_t)dc[b] != 0;
    return any;
}

// The decode front end's view of a copy of the reconstruction, so that its filter runs on it, and the record of macroblock mb at
// level `level` (> 0) as the decode front end's host half would leave it.
FL_VP8_HD Vp8DecPic vp8_lf_pic(const Vp8Pic &p, uint8_t *copy)
{
    Vp8DecPic d;
    d.recs = nullptr; d.lev = nullptr; d.dq = nullptr;
    d.mbw = p.mbw; d.mbh = p.mbh; d.nlevels = 0u; d.filter_type = 2u; // the normal filter
    d.y = copy;
    d.u = copy + (uint64_t)p.mbw * p.mbh * 256u;
    d.v = d.u + (uint64_t)p.mbw * p.mbh * 64u;
    return d;
}
template <bool I4> FL_VP8_HD Vp8MbRecord vp8_lf_record(const Vp8Pic &p, uint64_t mb, uint32_t level)
{
    Vp8MbRecord r{};
    uint8_t fs[3];
    vp8_filter_strength((int)level, 0, fs);
    r.f_limit = fs[0]; r.f_ilevel = fs[1]; r.hev_thresh = fs[2];
    r.inner = vp8_lf_inner<I4>(p, mb);
    return r;
}

// Item i of the cost: the squared difference of one visible sample, i < w h + 2 cw ch in the order of the source planes
// (under vp8_fits the count stays below 2^29)
FL_VP8_HD uint32_t vp8_lf_items(const Vp8Pic &p) { return p.w * p.h + 2u * p.cw * p.ch; }
FL_VP8_HD uint32_t vp8_lf_sq_diff(const Vp8Pic &p, const uint8_t *rec, uint32_t i)
{
    const uint32_t ysz = p.w * p.h, csz = p.cw * p.ch;
    uint64_t at;
    if (i < ysz) at = (uint64_t)(i / p.w) * (p.mbw * 16u) + i % p.w;
    else {
        const uint32_t k = i - ysz, pl = k >= csz ? 1u : 0u, j = k - pl * csz;
        at = (uint64_t)p.mbw * p.mbh * (256u + 64u * pl) + (uint64_t)(j / p.cw) * (p.mbw * 8u) + j % p.cw;
    }
    const int d = (int)rec[at] - (int)p.src[i];
    return (uint32_t)(d * d);
}

} // namespace fl
