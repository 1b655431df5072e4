// fl_vp8dec_core.h -- the lossy WebP decoder's arithmetic behind the boolean coder, as code that compiles for the host and for
// the device: dequantisation, inverse WHT / DCT (fl_vp8_core.h's), intra prediction of macroblocks and of 4x4 sub-blocks, the
// loop filters, the ALPH filters and libwebp's "fancy" up-sampling with its 14-bit YUV -> RGB.  fl_vp8dec.hip spreads the items
// of every step over lanes and macroblocks; tests/vp8_src_host.cpp runs the same functions in plain loops on the CPU.
// No HIP header is needed to include this one.
//
// The reconstruction lives in planes padded to whole macroblocks (Y 16 mbw x 16 mbh, then U and V 8 mbw x 8 mbh each); prediction
// reads its neighbours from there: 127 above the frame, 129 to its left, and past the last macroblock of a row the row's last
// sample again (the top-right rule of the last column).
#pragma once
#include <stdint.h>

#include "fl_vp8_core.h"
#include "fl_vp8_dtables.h"
#include "fl_vp8src.h"

namespace fl {

struct Vp8DecPic {
    const Vp8MbRecord *recs;
    const int16_t *lev;
    const uint16_t (*dq)[8];
    uint8_t *y, *u, *v;      // (no arrays: indexed by a plane number they would not stay in registers)
    uint32_t mbw, mbh, nlevels, filter_type;
};
FL_VP8_HD uint8_t *vp8d_plane(const Vp8DecPic &p, int pl) { return pl == 0 ? p.y : pl == 1 ? p.u : p.v; }
FL_VP8_HD uint32_t vp8d_stride(const Vp8DecPic &p, int pl) { return pl == 0 ? p.mbw * 16u : p.mbw * 8u; }

FL_VP8_HD void vp8d_pic(Vp8DecPic &p, const uint8_t *blob, uint8_t *planes)
{
    const Vp8BlobHeader *H = reinterpret_cast<const Vp8BlobHeader *>(blob);
    p.recs = reinterpret_cast<const Vp8MbRecord *>(blob + H->rec_off);
    p.lev = reinterpret_cast<const int16_t *>(blob + H->lev_off);
    p.dq = H->dq;
    p.mbw = H->mbw; p.mbh = H->mbh; p.nlevels = H->nlevels; p.filter_type = H->filter_type;
    p.y = planes;
    p.u = planes + (uint64_t)p.mbw * p.mbh * 256u;
    p.v = p.u + (uint64_t)p.mbw * p.mbh * 64u;
}

// One macroblock's working set between the steps: LDS on the device (one per wave), the stack on the host.
struct Vp8DecWork {
    int32_t res[24][16];  // what the inverse DCT leaves to add to the prediction, raster
    int32_t ydc[16];      // the luma blocks' DCs from the Y2 block
    int32_t dcv[3];       // the DC prediction's value per plane
    int32_t pad;
};

// sample (x, y) of a plane for prediction; x and y may be -1, x may pass the padded width
FL_VP8_HD int vp8d_sample(const Vp8DecPic &p, int pl, int x, int y)
{
    if (y < 0) return 127;
    if (x < 0) return 129;
    const int w = (int)vp8d_stride(p, pl);
    return vp8d_plane(p, pl)[(uint64_t)y * vp8d_stride(p, pl) + (uint32_t)(x < w ? x : w - 1)];
}

FL_VP8_HD uint32_t vp8d_cnt(const Vp8MbRecord &r, int b) { return r.cnt[b] > 16u ? 16u : r.cnt[b]; }

// the dequantised coefficients of block b (raster); like libwebp's, they are 16-bit
FL_VP8_HD void vp8d_dequant(const Vp8DecPic &p, const Vp8MbRecord &r, int b, int dc_step, int ac_step, int *in)
{
    uint32_t off = r.lev;
    for (int k = 0; k < b; ++k) off += vp8d_cnt(r, k);
    const uint32_t n = vp8d_cnt(r, b);
    for (int i = 0; i < 16; ++i) in[i] = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const int l = off + k < p.nlevels ? p.lev[off + k] : 0; // (a damaged blob: wrong pixels, no read past the levels)
        in[kVp8Zigzag[k]] = (int16_t)(l * (k ? ac_step : dc_step));
    }
}

// Step A, item k of 4: the Y2 block through the inverse WHT (0), the DC prediction's value of plane k - 1 (1..3)
FL_VP8_HD void vp8d_prepare(const Vp8DecPic &p, const Vp8MbRecord &r, Vp8DecWork &w, uint32_t mbx, uint32_t mby, uint32_t k)
{
    if (k == 0u) {
        if (r.ymode == kVp8BPred) return;
        const uint16_t *q = p.dq[r.segment & 3u];
        int in[16], dc[16];
        vp8d_dequant(p, r, 24, q[2], q[3], in);
        vp8_iwht(in, dc);
        for (int b = 0; b < 16; ++b) w.ydc[b] = (int16_t)dc[b];
        return;
    }
    const int pl = (int)k - 1, n = pl ? 8 : 16, sh = pl ? 3 : 4;
    const int x0 = (int)mbx * n, y0 = (int)mby * n;
    int st = 0, sl = 0;
    for (int i = 0; i < n; ++i) { st += vp8d_sample(p, pl, x0 + i, y0 - 1); sl += vp8d_sample(p, pl, x0 - 1, y0 + i); }
    w.dcv[pl] = mby && mbx ? (st + sl + n) >> (sh + 1) : mby ? (st + (n >> 1)) >> sh : mbx ? (sl + (n >> 1)) >> sh : 128;
}

// Step B, item = block b of 24: its residual
FL_VP8_HD void vp8d_residual(const Vp8DecPic &p, const Vp8MbRecord &r, Vp8DecWork &w, uint32_t b)
{
    const uint16_t *q = p.dq[r.segment & 3u];
    const bool i16 = r.ymode != kVp8BPred;
    int in[16], res[16];
    vp8d_dequant(p, r, (int)b, b < 16u ? q[0] : q[4], b < 16u ? q[1] : q[5], in);
    if (b < 16u && i16) in[0] = w.ydc[b];
    vp8_idct(in, res);
    for (int i = 0; i < 16; ++i) w.res[b][i] = res[i];
}

FL_VP8_HD int vp8d_avg2(int a, int b) { return (a + b + 1) >> 1; }
FL_VP8_HD int vp8d_avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }

// prediction of sample (x, y) of a 4x4 sub-block: T[0..7] the row above and above-right, L[0..3] the column to the left, P the corner
FL_VP8_HD int vp8d_predict4(int mode, int x, int y, const int *T, const int *L, int P)
{
    // E: the edge from the bottom of the left column over the corner to the end of the row above
    int E[13];
    E[0] = L[3]; E[1] = L[2]; E[2] = L[1]; E[3] = L[0]; E[4] = P;
    for (int i = 0; i < 8; ++i) E[5 + i] = T[i];
    switch (mode) {
    case VP8_B_DC: return (T[0] + T[1] + T[2] + T[3] + L[0] + L[1] + L[2] + L[3] + 4) >> 3;
    case VP8_B_TM: return vp8_clip8(T[x] + L[y] - P);
    case VP8_B_VE: return vp8d_avg3(E[4 + x], E[5 + x], E[6 + x]);
    case VP8_B_HE: return y < 3 ? vp8d_avg3(E[4 - y], E[3 - y], E[2 - y]) : vp8d_avg3(L[2], L[3], L[3]);
    case VP8_B_RD: { const int i = 4 + x - y; return vp8d_avg3(E[i - 1], E[i], E[i + 1]); }
    case VP8_B_LD: { const int i = x + y; return i < 6 ? vp8d_avg3(T[i], T[i + 1], T[i + 2]) : vp8d_avg3(T[6], T[7], T[7]); }
    case VP8_B_VR: {
        // rows 0 and 2: averages of two along the row above, rows 1 and 3 of three; each pair of rows shifts right by one
        const int i = 2 * x - y; // position on the edge in half steps, 0 = between the corner and T[0]
        if (i == -1) return vp8d_avg3(L[0], P, T[0]);
        if (i == -2) return vp8d_avg3(L[1], L[0], P);
        if (i == -3) return vp8d_avg3(L[2], L[1], L[0]);
        const int k = i >> 1; // E[4 + k], E[5 + k]
        return (i & 1) == 0 ? vp8d_avg2(E[4 + k], E[5 + k]) : vp8d_avg3(E[4 + k], E[5 + k], E[6 + k]);
    }
    case VP8_B_VL: {
        if (x == 3 && y >= 2) return y == 2 ? vp8d_avg3(T[4], T[5], T[6]) : vp8d_avg3(T[5], T[6], T[7]); // (the format's own exception)
        const int k = x + (y >> 1);
        return (y & 1) == 0 ? vp8d_avg2(T[k], T[k + 1]) : vp8d_avg3(T[k], T[k + 1], T[k + 2]);
    }
    case VP8_B_HD: {
        const int i = 2 * y - x; // half steps down the left column, 0 = between the corner and L[0]
        if (i == -1) return vp8d_avg3(L[0], P, T[0]);
        if (i == -2) return vp8d_avg3(P, T[0], T[1]);
        if (i == -3) return vp8d_avg3(T[0], T[1], T[2]);
        const int k = i >> 1; // E[4 - k], E[3 - k]
        return (i & 1) == 0 ? vp8d_avg2(E[4 - k], E[3 - k]) : vp8d_avg3(E[4 - k], E[3 - k], E[2 - k]);
    }
    default: { // VP8_B_HU
        const int i = 2 * y + x;
        if (i >= 6) return L[3];
        if (i == 5) return vp8d_avg3(L[2], L[3], L[3]);
        const int k = i >> 1;
        return (i & 1) == 0 ? vp8d_avg2(L[k], L[k + 1]) : vp8d_avg3(L[k], L[k + 1], L[k + 2]);
    }
    }
}

FL_VP8_HD int vp8d_predict_mb(const Vp8DecPic &p, const Vp8DecWork &w, int pl, int mode, int x0, int y0, int x, int y)
{
    switch (mode) {
    case VP8_DC: return w.dcv[pl];
    case VP8_V: return vp8d_sample(p, pl, x0 + x, y0 - 1);
    case VP8_H: return vp8d_sample(p, pl, x0 - 1, y0 + y);
    default: return vp8_clip8(vp8d_sample(p, pl, x0 + x, y0 - 1) + vp8d_sample(p, pl, x0 - 1, y0 + y) - vp8d_sample(p, pl, x0 - 1, y0 - 1));
    }
}

// Step C, sub-step s of 16, lane of 64.  Sub-step 0: the chroma planes (two samples a lane) and the luma of a macroblock with
// one mode (four a lane).  A B_PRED macroblock: sub-block s in every sub-step, one sample a lane on lanes 0..15 -- sub-block s
// predicts from the ones before it, so a barrier separates the sub-steps.
constexpr uint32_t kVp8dSubSteps = 16, kVp8dLanes = 64;
FL_VP8_HD void vp8d_reconstruct(const Vp8DecPic &p, const Vp8MbRecord &r, const Vp8DecWork &w, uint32_t mbx, uint32_t mby, uint32_t s, uint32_t lane)
{
    if (s == 0u) {
        for (uint32_t i = lane; i < 128u; i += kVp8dLanes) {
            const int pl = 1 + (int)(i >> 6), x = (int)(i & 7u), y = (int)((i >> 3) & 7u);
            const int v = vp8d_predict_mb(p, w, pl, r.uvmode & 3u, (int)mbx * 8, (int)mby * 8, x, y) + w.res[16 + (pl - 1) * 4 + (y >> 2) * 2 + (x >> 2)][(y & 3) * 4 + (x & 3)];
            vp8d_plane(p, pl)[((uint64_t)mby * 8u + (uint32_t)y) * vp8d_stride(p, pl) + mbx * 8u + (uint32_t)x] = (uint8_t)vp8_clip8(v);
        }
        if (r.ymode != kVp8BPred)
            for (uint32_t i = lane; i < 256u; i += kVp8dLanes) {
                const int x = (int)(i & 15u), y = (int)(i >> 4);
                const int v = vp8d_predict_mb(p, w, 0, r.ymode & 3u, (int)mbx * 16, (int)mby * 16, x, y) + w.res[(y >> 2) * 4 + (x >> 2)][(y & 3) * 4 + (x & 3)];
                vp8d_plane(p, 0)[((uint64_t)mby * 16u + (uint32_t)y) * vp8d_stride(p, 0) + mbx * 16u + (uint32_t)x] = (uint8_t)vp8_clip8(v);
            }
    }
    if (r.ymode != kVp8BPred || lane >= 16u) return;
    const int bx = (int)(s & 3u) * 4, by = (int)(s >> 2) * 4, x = (int)(lane & 3u), y = (int)(lane >> 2);
    const int ax = (int)mbx * 16 + bx, ay = (int)mby * 16 + by;
    int T[8], L[4];
    for (int i = 0; i < 4; ++i) { T[i] = vp8d_sample(p, 0, ax + i, ay - 1); L[i] = vp8d_sample(p, 0, ax - 1, ay + i); }
    // above-right: of the sub-blocks in the macroblock's last column, all four rows take the samples above the macroblock to the right
    const int ty = bx == 12 ? (int)mby * 16 - 1 : ay - 1;
    for (int i = 4; i < 8; ++i) T[i] = vp8d_sample(p, 0, ax + i, ty);
    const int P = vp8d_sample(p, 0, ax - 1, ay - 1);
    const int mode = (r.bmodes[s >> 1] >> (4u * (s & 1u))) & 15;
    const int v = vp8d_predict4(mode < VP8_B_MODES ? mode : 0, x, y, T, L, P) + w.res[s][y * 4 + x];
    vp8d_plane(p, 0)[(uint64_t)(ay + y) * vp8d_stride(p, 0) + (uint32_t)(ax + x)] = (uint8_t)vp8_clip8(v);
}

// ---- loop filter (section 15) -------------------------------------------------------------------------------------------------
FL_VP8_HD int vp8d_abs(int v) { return v < 0 ? -v : v; }
FL_VP8_HD int vp8d_sclip1(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }
FL_VP8_HD int vp8d_sclip2(int v) { return v < -16 ? -16 : v > 15 ? 15 : v; }

// One line across an edge: q points at the first sample behind it, step leads across it.  kind: 0 = simple, 1 = inner edge of the
// normal filter, 2 = macroblock edge of the normal filter.
FL_VP8_HD void vp8d_filter_line(uint8_t *q, int64_t step, int kind, int thresh2, int ilevel, int hev_thresh)
{
    const int p1 = q[-2 * step], p0 = q[-step], q0 = q[0], q1 = q[step];
    if (4 * vp8d_abs(p0 - q0) + vp8d_abs(p1 - q1) > thresh2) return;
    if (kind == 0) {
        const int a = 3 * (q0 - p0) + vp8d_sclip1(p1 - q1);
        const int a1 = vp8d_sclip2((a + 4) >> 3), a2 = vp8d_sclip2((a + 3) >> 3);
        q[-step] = (uint8_t)vp8_clip8(p0 + a2); q[0] = (uint8_t)vp8_clip8(q0 - a1);
        return;
    }
    const int p3 = q[-4 * step], p2 = q[-3 * step], q2 = q[2 * step], q3 = q[3 * step];
    if (vp8d_abs(p3 - p2) > ilevel || vp8d_abs(p2 - p1) > ilevel || vp8d_abs(p1 - p0) > ilevel || vp8d_abs(q3 - q2) > ilevel ||
        vp8d_abs(q2 - q1) > ilevel || vp8d_abs(q1 - q0) > ilevel) return;
    if (vp8d_abs(p1 - p0) > hev_thresh || vp8d_abs(q1 - q0) > hev_thresh) { // high edge variance: the two samples at the edge only
        const int a = 3 * (q0 - p0) + vp8d_sclip1(p1 - q1);
        const int a1 = vp8d_sclip2((a + 4) >> 3), a2 = vp8d_sclip2((a + 3) >> 3);
        q[-step] = (uint8_t)vp8_clip8(p0 + a2); q[0] = (uint8_t)vp8_clip8(q0 - a1);
    } else if (kind == 1) {
        const int a = 3 * (q0 - p0);
        const int a1 = vp8d_sclip2((a + 4) >> 3), a2 = vp8d_sclip2((a + 3) >> 3), a3 = (a1 + 1) >> 1;
        q[-2 * step] = (uint8_t)vp8_clip8(p1 + a3); q[-step] = (uint8_t)vp8_clip8(p0 + a2);
        q[0] = (uint8_t)vp8_clip8(q0 - a1); q[step] = (uint8_t)vp8_clip8(q1 - a3);
    } else {
        const int a = vp8d_sclip1(3 * (q0 - p0) + vp8d_sclip1(p1 - q1));
        const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
        q[-3 * step] = (uint8_t)vp8_clip8(p2 + a3); q[-2 * step] = (uint8_t)vp8_clip8(p1 + a2); q[-step] = (uint8_t)vp8_clip8(p0 + a1);
        q[0] = (uint8_t)vp8_clip8(q0 - a1); q[step] = (uint8_t)vp8_clip8(q1 - a2); q[2 * step] = (uint8_t)vp8_clip8(q2 - a3);
    }
}

// The filter of one macroblock in eight steps -- left edge, inner vertical edges at 4 / 8 / 12, top edge, inner horizontal edges
// at 4 / 8 / 12 -- each step 32 lines: lanes 0..15 luma, 16..23 U, 24..31 V (chroma has one inner edge, at 4; the simple filter
// leaves chroma alone).  The edges of a macroblock overlap, so a barrier separates the steps.
constexpr uint32_t kVp8dFilterSteps = 8, kVp8dFilterLanes = 32;
FL_VP8_HD void vp8d_filter(const Vp8DecPic &p, const Vp8MbRecord &r, uint32_t mbx, uint32_t mby, uint32_t s, uint32_t lane)
{
    if (!p.filter_type || !r.f_limit) return;
    const bool horizontal = s >= 4u; // the edge runs horizontally: lines go down across it
    const uint32_t e = s & 3u;       // 0 = the macroblock's own edge, 1..3 inner
    if (e == 0u ? (horizontal ? mby == 0u : mbx == 0u) : !r.inner) return;
    const int pl = lane < 16u ? 0 : lane < 24u ? 1 : 2;
    if (pl && (p.filter_type == 1u || e > 1u)) return;
    const uint32_t n = pl ? 8u : 16u, i = pl ? (lane - 16u) & 7u : lane;
    const uint32_t x = mbx * n + (horizontal ? i : e * 4u), y = mby * n + (horizontal ? e * 4u : i);
    uint8_t *q = vp8d_plane(p, pl) + (uint64_t)y * vp8d_stride(p, pl) + x;
    const int limit = e == 0u ? r.f_limit + 4 : r.f_limit;
    vp8d_filter_line(q, horizontal ? (int64_t)vp8d_stride(p, pl) : 1, p.filter_type == 1u ? 0 : e == 0u ? 2 : 1, 2 * limit + 1, r.f_ilevel, r.hev_thresh);
}

// ---- ALPH filters ---------------------------------------------------------------------------------------------------------------
// the gradient filter's sample (x, y) from the ones before it (in: the chunk's value there, out: the plane)
FL_VP8_HD uint8_t vp8d_alpha_gradient(uint8_t in, const uint8_t *out, uint32_t w, uint32_t x, uint32_t y)
{
    const uint64_t at = (uint64_t)y * w + x;
    int pred;
    if (y == 0u) pred = x ? out[at - 1u] : 0;
    else if (x == 0u) pred = out[at - w];
    else pred = vp8_clip8((int)out[at - 1u] + (int)out[at - w] - (int)out[at - w - 1u]);
    return (uint8_t)(in + pred);
}

// ---- planes to pixels -------------------------------------------------------------------------------------------------------------
FL_VP8_HD int vp8d_clip14(int v) { return (v & ~16383) == 0 ? v >> 6 : v < 0 ? 0 : 255; }

// the up-sampled chroma at column X from the chroma row nearer to the luma row (n) and the farther one (f), cw samples each
FL_VP8_HD int vp8d_upsample(const uint8_t *n, const uint8_t *f, uint32_t X, uint32_t w, uint32_t cw)
{
    if (X == 0u) return (3 * n[0] + f[0] + 2) >> 2;
    if (X == w - 1u && !(w & 1u)) return (3 * n[cw - 1u] + f[cw - 1u] + 2) >> 2;
    const uint32_t a = X >> 1, b = (X & 1u) ? a + 1u : a - 1u; // the nearer column and the other one
    return (((n[a] + n[b] + f[a] + f[b] + 8 + 2 * (n[b] + f[a])) >> 3) + n[a]) >> 1;
}

// pixel (X, Y) of the w x h picture: R, G, B to d[0 .. 3), and d[3] = the alpha plane's sample or 255 where channels == 4
FL_VP8_HD void vp8d_pixel(const Vp8DecPic &p, const uint8_t *alpha, uint32_t w, uint32_t h, uint32_t channels, uint32_t X, uint32_t Y, uint8_t *d)
{
    const uint32_t cw = (w + 1u) >> 1, ch = (h + 1u) >> 1;
    // luma row Y lies between chroma rows (Y - 1) / 2 and (Y + 1) / 2 and nearer to Y / 2; outside the picture: the nearer one again
    uint32_t rn = Y >> 1, rf = Y == 0u ? 0u : (Y & 1u) ? rn + 1u : rn - 1u;
    if (rf >= ch) rf = rn;
    int uv[2];
    for (int c = 0; c < 2; ++c) {
        const uint8_t *pl = c ? p.v : p.u;
        uv[c] = vp8d_upsample(pl + (uint64_t)rn * vp8d_stride(p, 1), pl + (uint64_t)rf * vp8d_stride(p, 1), X, w, cw);
    }
    const int y = vp8d_plane(p, 0)[(uint64_t)Y * vp8d_stride(p, 0) + X], yy = (y * 19077) >> 8;
    d[0] = (uint8_t)vp8d_clip14(yy + ((uv[1] * 26149) >> 8) - 14234);
    d[1] = (uint8_t)vp8d_clip14(yy - ((uv[0] * 6419) >> 8) - ((uv[1] * 13320) >> 8) + 8708);
    d[2] = (uint8_t)vp8d_clip14(yy + ((uv[0] * 33050) >> 8) - 17685);
    if (channels == 4u) d[3] = alpha ? alpha[(uint64_t)Y * w + X] : 255;
}

} // namespace fl
