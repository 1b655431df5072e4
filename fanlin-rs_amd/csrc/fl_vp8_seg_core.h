// fl_vp8_seg_core.h -- segment-adaptive quantisers of the lossy WebP encoder (FLGPU_FEO_SEGMENTS on any of the eight lossy front ends):
// the rule that sorts a picture's macroblocks into up to four classes by activity and gives each class its quantiser index, as code
// that compiles for the host and for the device.  fl_vp8_core.h holds the record the rule leaves (Vp8SegRec), the header and the ids
// in partition 0 (vp8_put_first_partition) and the limits; the analysis takes each macroblock's steps from its class (vp8_seg_pick).
// tests/vp8_seg_model.py restates the rule, tests/vp8_host.cpp runs it in plain loops, fl_vp8.hip (vp8_segment_kernel) over a
// workgroup.
//
// The rule, integer only.  Inputs: the luma plane padded to whole macroblocks by edge replication (as vp8_phase_load pads it) and the
// picture's base index qi = vp8_quality_index(quality).
//   1. activity of a macroblock: act = sum over its 256 samples of |Y - m|, m = (sum Y + 128) >> 8;
//   2. bin = min(255, act >> kVp8SegBinShift);
//   3. macroblocks of bin 0 are flat: they stay out of steps 4-6 and belong to class 0.  No non-flat macroblock, or one occupied bin
//      among them: no segmentation;
//   4. histogram over bins 1..255; lo, hi = the least and greatest occupied bin; centres c_k = lo + (2 k + 1)(hi - lo) / 8, k = 0..3;
//   5. six rounds: every bin of [lo, hi] goes to the class with the least |a - c_k| (ties: the lowest k); c_k = (sum a hist[a] +
//      n_k / 2) / n_k where n_k > 0, else unchanged.  Then one more assignment with the final centres;
//   6. mid = (sum c_k n_k + N / 2) / N over the non-flat macroblocks; amp = max(1, (kVp8SegAmpNum qi) >> 3); off_k = (c_k - mid) amp /
//      kVp8SegSpan towards zero, clamped to +-amp; qi_k = clamp(qi + off_k, 0, 127);
//   7. a class with a macroblock is used (flat ones count in class 0).  Every used class at qi: no segmentation, the twin's file;
//   8. the tree's probabilities from the class counts n0..n3 (flat ones in n0): (left, right) = (n0 + n1, n2 + n3), (n0, n1),
//      (n2, n3); 255 if right == 0, else clamp((255 left + (l + r) / 2) / (l + r), 1, 255).
#pragma once
#include "fl_vp8_core.h"

namespace fl {

constexpr uint32_t kVp8SegBinShift = 5;   // activity per bin: 32, an eighth of a grey level of mean deviation per sample
constexpr uint32_t kVp8SegAmpNum = 3;     // the largest offset: 3/8 of the base index
constexpr int32_t kVp8SegSpan = 96;       // the distance in bins from the mean centre at which the offset reaches it
constexpr uint32_t kVp8SegRounds = 6;
constexpr uint32_t kVp8SegBins = 256;

// Step 1, one sample's share: |Y - m|; and the mean from the sum of the 256 samples
FL_VP8_HD uint32_t vp8_seg_mean(uint32_t sum) { return (sum + 128u) >> 8; }
FL_VP8_HD uint32_t vp8_seg_dev(uint32_t y, uint32_t m) { return y > m ? y - m : m - y; }
// Step 2
FL_VP8_HD uint32_t vp8_seg_bin(uint32_t act) { const uint32_t b = act >> kVp8SegBinShift; return b > 255u ? 255u : b; }
// sample k of 256 of macroblock (mbx, mby) of an unpadded w x h plane, coordinates clamped
FL_VP8_HD uint32_t vp8_seg_sample(const uint8_t *y, uint32_t w, uint32_t h, uint32_t mbx, uint32_t mby, uint32_t k)
{
    uint32_t x = mbx * 16u + (k & 15u), yy = mby * 16u + (k >> 4);
    x = x < w ? x : w - 1u; yy = yy < h ? yy : h - 1u;
    return y[(uint64_t)yy * w + x];
}

// Step 4: centre k of the range
FL_VP8_HD int32_t vp8_seg_centre0(uint32_t lo, uint32_t hi, uint32_t k) { return (int32_t)(lo + ((2u * k + 1u) * (hi - lo)) / 8u); }
// Step 5: the class of bin a; the centre of a class from its sums
FL_VP8_HD uint32_t vp8_seg_nearest(int32_t a, const int32_t *c)
{
    uint32_t best = 0;
    int32_t bd = a > c[0] ? a - c[0] : c[0] - a;
    for (uint32_t k = 1; k < 4u; ++k) {
        const int32_t d = a > c[k] ? a - c[k] : c[k] - a;
        if (d < bd) { bd = d; best = k; }
    }
    return best;
}
FL_VP8_HD int32_t vp8_seg_centre(uint32_t sum, uint32_t n, int32_t old) { return n ? (int32_t)((sum + n / 2u) / n) : old; }

// Steps 6-8 from the final centres c, the non-flat counts n of the final assignment, the number of flat macroblocks and qi
FL_VP8_HD uint32_t vp8_seg_tree_prob(uint32_t left, uint32_t right)
{
    if (right == 0u) return 255u;
    const uint64_t t = (uint64_t)left + right, v = (255u * (uint64_t)left + t / 2u) / t;
    return v < 1u ? 1u : v > 255u ? 255u : (uint32_t)v;
}
FL_VP8_HD void vp8_seg_finish(Vp8SegRec &r, const int32_t *c, const uint32_t *n, uint32_t flat, uint32_t qi)
{
    const uint64_t N = (uint64_t)n[0] + n[1] + n[2] + n[3];
    uint64_t s = 0;
    for (int k = 0; k < 4; ++k) s += (uint64_t)c[k] * n[k];
    const int32_t mid = N ? (int32_t)((s + N / 2u) / N) : 0;
    const int32_t amp = (int32_t)((kVp8SegAmpNum * qi) >> 3) < 1 ? 1 : (int32_t)((kVp8SegAmpNum * qi) >> 3);
    const uint32_t cnt[4] = {n[0] + flat, n[1], n[2], n[3]};
    bool on = false;
    for (int k = 0; k < 4; ++k) {
        int32_t off = (c[k] - mid) * amp / kVp8SegSpan; // (C++ division truncates towards zero)
        off = off < -amp ? -amp : off > amp ? amp : off;
        const int32_t q = (int32_t)qi + off;
        r.qi[k] = (uint8_t)(q < 0 ? 0 : q > 127 ? 127 : q);
        on |= N != 0u && cnt[k] != 0u && r.qi[k] != qi;
    }
    r.prob[0] = (uint8_t)vp8_seg_tree_prob(cnt[0] + cnt[1], cnt[2] + cnt[3]);
    r.prob[1] = (uint8_t)vp8_seg_tree_prob(cnt[0], cnt[1]);
    r.prob[2] = (uint8_t)vp8_seg_tree_prob(cnt[2], cnt[3]);
    r.on = on;
    if (!on) { for (int k = 0; k < 4; ++k) r.qi[k] = (uint8_t)qi; r.prob[0] = r.prob[1] = r.prob[2] = 255; }
}

// The whole rule in plain loops, on a histogram of the macroblocks' bins: the record, and cls[a] = the class of bin a (0 for every
// bin where the picture is not segmented).  The device kernel runs the same steps over a workgroup.
FL_VP8_HD void vp8_seg_classify(const uint32_t *hist, uint32_t qi, Vp8SegRec &r, uint8_t *cls)
{
    for (uint32_t a = 0; a < kVp8SegBins; ++a) cls[a] = 0;
    uint32_t lo = kVp8SegBins, hi = 0;
    for (uint32_t a = 1; a < kVp8SegBins; ++a) if (hist[a]) { if (a < lo) lo = a; hi = a; }
    int32_t c[4] = {0, 0, 0, 0};
    uint32_t n[4] = {0, 0, 0, 0};
    if (lo >= hi) { vp8_seg_finish(r, c, n, 0u, qi); return; } // none, or a single occupied bin (n = 0: not segmented)
    for (uint32_t k = 0; k < 4u; ++k) c[k] = vp8_seg_centre0(lo, hi, k);
    for (uint32_t round = 0; round <= kVp8SegRounds; ++round) {
        uint32_t sum[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) n[k] = 0;
        for (uint32_t a = lo; a <= hi; ++a) {
            const uint32_t k = vp8_seg_nearest((int32_t)a, c);
            cls[a] = (uint8_t)k;
            n[k] += hist[a]; sum[k] += a * hist[a];
        }
        if (round < kVp8SegRounds) for (int k = 0; k < 4; ++k) c[k] = vp8_seg_centre(sum[k], n[k], c[k]);
    }
    vp8_seg_finish(r, c, n, hist[0], qi);
    if (!r.on) for (uint32_t a = 0; a < kVp8SegBins; ++a) cls[a] = 0;
}

// The bins of a picture's macroblocks, in plain loops (the host twin's phase A): map[mb] = bin, hist[bin] counted
FL_VP8_HD void vp8_seg_bins(const uint8_t *y, uint32_t w, uint32_t h, uint8_t *map, uint32_t *hist)
{
    const uint32_t mbw = vp8_mbs(w), mbh = vp8_mbs(h);
    for (uint32_t a = 0; a < kVp8SegBins; ++a) hist[a] = 0;
    for (uint32_t mby = 0; mby < mbh; ++mby)
        for (uint32_t mbx = 0; mbx < mbw; ++mbx) {
            uint32_t sum = 0, act = 0;
            for (uint32_t k = 0; k < 256u; ++k) sum += vp8_seg_sample(y, w, h, mbx, mby, k);
            const uint32_t m = vp8_seg_mean(sum);
            for (uint32_t k = 0; k < 256u; ++k) act += vp8_seg_dev(vp8_seg_sample(y, w, h, mbx, mby, k), m);
            const uint32_t b = vp8_seg_bin(act);
            map[(uint64_t)mby * mbw + mbx] = (uint8_t)b;
            ++hist[b];
        }
}

} // namespace fl
