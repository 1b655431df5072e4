// fl_vp8_i4_core.h -- the I4 variant of the lossy WebP encoder (FLGPU_FE_WEBP_LOSSY_I4): the analysis phases that try a macroblock's
// luma as sixteen 4x4 sub-blocks, decide between that and I16, and commit the winner.  fl_vp8_core.h states the rule and holds
// everything else (bounds, penalty, transforms, the coder with its mode tree); the ten predictors are the decoder's
// (fl_vp8dec_core.h vp8d_predict4), not a second copy.  Like fl_vp8_core.h this compiles for the host and the device: fl_vp8.hip
// spreads the items of every phase over the lanes of a wave, tests/vp8_host.cpp runs them in plain loops.
#pragma once
#include <stdint.h>

#include "fl_vp8_core.h"
#include "fl_vp8dec_core.h"

namespace fl {

// the ten modes in the format's numbering (the order ties are broken in), as fl_vp8_dtables.h's numbers
constexpr uint8_t kVp8I4Order[10] = {VP8_B_DC, VP8_B_TM, VP8_B_VE, VP8_B_HE, VP8_B_LD, VP8_B_RD, VP8_B_VR, VP8_B_VL, VP8_B_HD, VP8_B_HU};

// The I4 trial's working set beside Vp8Mb: LDS on the device, the stack on the host.
struct Vp8I4 {
    int32_t T[8], L[4], P;          // the current sub-block's neighbours: above and above-right, left, corner
    int32_t a[16], t[16], c[16];    // residual / dequantised levels, a transform's first pass, coefficients / inverse DCT (raster)
    uint32_t sse[10];               // the current sub-block's ten SSEs, in the format's numbering
    uint32_t s4, pick;              // the sum of the chosen SSEs so far; the current sub-block's choice (index into kVp8I4Order)
    int16_t lev[256];               // sixteen blocks' levels in coding order
    uint8_t wrk[256];               // the luma reconstruction so far, 16 x 16
    uint8_t pred[10][16];           // the current sub-block's ten predictions
    uint8_t tr[4];                  // the four samples above and to the right of the macroblock
    uint8_t mode[16], nz[16];
};

// Item k of 5: the macroblock's above-right samples (the row above, of the macroblock to the right; past the frame's right edge
// that row's last sample; 127 above the frame), and S4 = 0.
FL_VP8_HD void vp8_i4_phase_begin(const Vp8Pic &p, Vp8I4 &w, uint32_t mbx, uint32_t mby, uint32_t k)
{
    if (k == 4u) { w.s4 = 0u; return; }
    const uint64_t rys = (uint64_t)p.mbw * 16u;
    uint64_t x = (uint64_t)mbx * 16u + 16u + k;
    if (x > rys - 1u) x = rys - 1u;
    w.tr[k] = mby == 0u ? 127 : p.rec[((uint64_t)mby * 16u - 1u) * rys + x];
}
constexpr uint32_t kVp8I4BeginItems = 5;

// Sub-block s, item k of 13: its neighbours, from the working copy inside the macroblock and from Vp8Mb's borders outside.  The
// sub-blocks of the last column take their above-right from above the macroblock in every row, as the decoder does.
FL_VP8_HD void vp8_i4_phase_edges(const Vp8Mb &m, Vp8I4 &w, uint32_t s, uint32_t k)
{
    const uint32_t bx = (s & 3u) * 4u, by = (s >> 2) * 4u;
    if (k < 8u) {
        const uint32_t x = bx + k;
        w.T[k] = x >= 16u ? w.tr[x - 16u] : by == 0u ? m.top[0][1u + x] : w.wrk[(by - 1u) * 16u + x];
    } else if (k < 12u) {
        const uint32_t y = by + k - 8u;
        w.L[k - 8u] = bx == 0u ? m.left[0][y] : w.wrk[y * 16u + bx - 1u];
    } else
        w.P = by == 0u ? m.top[0][bx] : bx == 0u ? m.left[0][by - 1u] : w.wrk[(by - 1u) * 16u + bx - 1u];
}
constexpr uint32_t kVp8I4EdgeItems = 13;

// Sub-block s, item k of 160: sample k % 16 of prediction k / 16; returns its squared error, which the caller sums per mode into
// w.sse
FL_VP8_HD uint32_t vp8_i4_phase_predict(const Vp8Mb &m, Vp8I4 &w, uint32_t s, uint32_t k)
{
    const uint32_t mi = k >> 4, i = k & 15u, x = i & 3u, y = i >> 2;
    const int v = vp8d_predict4(kVp8I4Order[mi], (int)x, (int)y, w.T, w.L, w.P);
    w.pred[mi][i] = (uint8_t)v;
    const int d = (int)m.src[((s >> 2) * 4u + y) * 16u + (s & 3u) * 4u + x] - v;
    return (uint32_t)(d * d);
}
constexpr uint32_t kVp8I4PredictItems = 160;

// Sub-block s (one item): the mode.  A later one replaces an earlier one only if it is strictly better.
FL_VP8_HD void vp8_i4_phase_pick(Vp8I4 &w, uint32_t s)
{
    uint32_t best = 0xffffffffu, pick = 0;
    for (uint32_t mi = 0; mi < 10u; ++mi)
        if (w.sse[mi] < best) { best = w.sse[mi]; pick = mi; }
    w.pick = pick;
    w.mode[s] = kVp8I4Order[pick];
    w.s4 += best;
}

// Sub-block s, the chosen mode's residual through transform, quantiser and back, every step's items independent of each other:
// residual (i of 16), forward rows (i of 4), forward columns (i of 4), quantise (coding position i of 16), inverse columns (i of 4),
// inverse rows (i of 4), reconstruct (i of 16).
FL_VP8_HD void vp8_i4_phase_residual(const Vp8Mb &m, Vp8I4 &w, uint32_t s, uint32_t i)
{
    w.a[i] = (int)m.src[((s >> 2) * 4u + (i >> 2)) * 16u + (s & 3u) * 4u + (i & 3u)] - (int)w.pred[w.pick][i];
}
FL_VP8_HD void vp8_i4_phase_fdct_rows(Vp8I4 &w, uint32_t i) { vp8_fdct_row(w.a, w.t, (int)i); }
FL_VP8_HD void vp8_i4_phase_fdct_cols(Vp8I4 &w, uint32_t i) { vp8_fdct_col(w.t, w.c, (int)i); }
FL_VP8_HD void vp8_i4_phase_quant(const Vp8Pic &p, Vp8I4 &w, uint32_t s, uint32_t i)
{
    const int r = kVp8Zigzag[i], step = i ? p.q.y1_ac : p.q.y1_dc;
    const int l = vp8_quantise(w.c[r], step, i == 0u);
    w.lev[s * 16u + i] = (int16_t)l;
    w.a[r] = l * step;
}
FL_VP8_HD void vp8_i4_phase_idct_cols(Vp8I4 &w, uint32_t i) { vp8_idct_col(w.a, w.t, (int)i); }
FL_VP8_HD void vp8_i4_phase_idct_rows(Vp8I4 &w, uint32_t i) { vp8_idct_row(w.t, w.c, (int)i); }
FL_VP8_HD void vp8_i4_phase_recon(Vp8I4 &w, uint32_t s, uint32_t i)
{
    w.wrk[((s >> 2) * 4u + (i >> 2)) * 16u + (s & 3u) * 4u + (i & 3u)] = (uint8_t)vp8_clip8((int)w.pred[w.pick][i] + w.c[i]);
    if (i == 0u) {
        int any = 0;
        for (uint32_t k = 0; k < 16u; ++k) any |= w.lev[s * 16u + k];
        w.nz[s] = any != 0;
    }
}

// S16, the I16 trial's luma SSE (after vp8_phase_modes), and the decision (after the I4 trial)
FL_VP8_HD uint32_t vp8_i4_s16(const Vp8Mb &m)
{
    uint32_t s = 0;
    for (int b = 0; b < 16; ++b) s += m.sse_y[m.ymode * 16 + b];
    return s;
}
// whether the I4 trial can win at all: S4 >= 0
FL_VP8_HD bool vp8_i4_worth_trying(const Vp8Pic &p, uint32_t s16) { return vp8_i4_penalty(p.q.y1_ac) < s16; }
FL_VP8_HD bool vp8_i4_wins(const Vp8Pic &p, const Vp8I4 &w, uint32_t s16) { return (uint64_t)w.s4 + vp8_i4_penalty(p.q.y1_ac) < s16; }

// The I4 trial won, item k of 273: the working copy goes to the picture, the levels and flags to Vp8Mb where vp8_phase_store
// expects them; there is no Y2 block.  The chroma blocks then go through vp8_phase_fdct and vp8_phase_recon as ever.
FL_VP8_HD void vp8_i4_phase_commit(const Vp8Pic &p, Vp8Mb &m, const Vp8I4 &w, uint32_t mbx, uint32_t mby, uint32_t k)
{
    if (k < 256u) {
        p.rec[((uint64_t)mby * 16u + (k >> 4)) * ((uint64_t)p.mbw * 16u) + (uint64_t)mbx * 16u + (k & 15u)] = w.wrk[k];
        m.lev[k] = w.lev[k];
    } else if (k < 272u) {
        m.lev[24u * 16u + k - 256u] = 0;
        m.nz[k - 256u] = w.nz[k - 256u];
    } else { m.nz[24] = 0; m.ymode = VP8_DC; }
}
constexpr uint32_t kVp8I4CommitItems = 273;

// Instead of vp8_phase_store, item k of kVp8MbLevels + 2: the levels, the record with the Y2 context a B_PRED macroblock passes
// on, and the mode record.
FL_VP8_HD void vp8_i4_phase_store(const Vp8Pic &p, const Vp8Mb &m, const Vp8I4 &w, bool i4, uint32_t mbx, uint32_t mby, uint32_t k)
{
    const uint64_t mb = (uint64_t)mby * p.mbw + mbx;
    if (k < kVp8MbLevels) { p.lev[mb * kVp8MbLevels + k] = m.lev[k]; return; }
    if (k == kVp8MbLevels) {
        uint32_t nz = 0;
        for (int b = 0; b < 25; ++b) nz |= (uint32_t)m.nz[b] << b;
        if (i4) {
            if (mbx) nz |= ((p.info[mb - 1u] >> 28) & 1u) << 24;
            if (mby) nz |= ((p.info[mb - p.mbw] >> (vp8_is_i4(p, mb - p.mbw) ? 29 : 28)) & 1u) << 25;
        }
        p.info[mb] = (uint32_t)m.ymode | (uint32_t)m.uvmode << 2 | nz << 4;
        return;
    }
    uint32_t lo = 0, hi = 0;
    for (uint32_t b = 0; b < 8u; ++b) {
        lo |= (i4 ? (uint32_t)w.mode[b] : kVp8BmI16 + vp8_context_mode(m.ymode)) << (4u * b);
        hi |= (i4 ? (uint32_t)w.mode[8u + b] : kVp8BmI16 + vp8_context_mode(m.ymode)) << (4u * b);
    }
    p.bm[2u * mb] = lo; p.bm[2u * mb + 1u] = hi;
}
constexpr uint32_t kVp8I4StoreItems = kVp8MbLevels + 2;

} // namespace fl
