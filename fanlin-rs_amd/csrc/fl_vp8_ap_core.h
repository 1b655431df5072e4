// fl_vp8_ap_core.h -- the adaptive-probability variants of the lossy WebP encoder (FLGPU_FE_WEBP_LOSSY_AP, FLGPU_FE_WEBP_LOSSY_I4_AP):
// the counting sink of the token walk and the rule that turns a picture's counts into its coefficient probability table.  Host and
// device code like fl_vp8_core.h, which holds the walk itself (vp8_put_block), the header's update flags
// (vp8_put_first_partition<I4, true>) and the limits; tests/vp8_ap_model.py restates the rule, tests/vp8_host.cpp runs it in
// plain loops.
//
// Counts.  For every coded macroblock (vp8_coded<I4> != 0) the walk that vp8_put_mb codes runs into a Vp8Count instead of a
// Vp8Bool: every boolean whose probability is entry i of the table [type 4][band 8][ctx 3][node 11] adds one to z[i] (a zero) or
// o[i] (a one), with the contexts the coder uses (a B_PRED macroblock's Y2 pass-through bits, block type 3 from coefficient 0).
// Sign bits, the categories' extra bits and everything in partition 0 are not counted.
// Candidate (the probability of a zero): 255 if o == 0, else (255 z + (z + o) / 2) / (z + o) clamped to 1..255.
// Decision, with u = kVp8CoefUpdateProb[i], C = kVp8BitCost and 64-bit sums (a picture at the macroblock limit visits a node
// millions of times at up to 2048 each): entry i becomes p_new iff z + o > 0, p_new != p_old and
//     z C[p_new] + o C[256 - p_new] + C[256 - u] + 8 x 256  <  z C[p_old] + o C[256 - p_old] + C[u]
// -- the tokens' cost with the new value plus the flag and the literal against their cost with the default and the flag.
#pragma once
#include "fl_vp8_core.h"

namespace fl {

constexpr uint32_t kVp8CoefProbs = 4 * 8 * 3 * 11;   // 1056 entries
constexpr uint32_t kVp8CountWords = 2 * kVp8CoefProbs; // z[1056] then o[1056]
static_assert(sizeof(kVp8CoefProb) == kVp8CoefProbs && sizeof(kVp8CoefUpdateProb) == kVp8CoefProbs, "one update flag per entry");

// The counting sink on the host: cnt[i] zeros, cnt[kVp8CoefProbs + i] ones of entry i; `tab` is the table the walk was given.
// (fl_vp8.hip has the same sink with LDS atomics.)
struct Vp8Count {
    const uint8_t *tab;
    uint32_t *cnt;
    FL_VP8_HD void node(int bit, const uint8_t *p) { ++cnt[(bit ? kVp8CoefProbs : 0u) + (uint32_t)(p - tab)]; }
    FL_VP8_HD void put(int, uint32_t) {}
};

// item k of kVp8MbBlocks x macroblocks: block k % 25 of macroblock k / 25 (a skipped macroblock and a B_PRED one's Y2 item count nothing)
template <bool I4, class Sink> FL_VP8_HD void vp8_ap_count_item(Sink &s, const Vp8Pic &p, uint32_t k)
{
    const uint32_t mb = k / kVp8MbBlocks, b = k % kVp8MbBlocks;
    const Vp8MbCtx c = vp8_mb_ctx<I4>(p, mb % p.mbw, mb / p.mbw);
    if (c.coded) vp8_put_mb_block(s, p.prob, c, b);
}

FL_VP8_HD uint32_t vp8_ap_candidate(uint32_t z, uint32_t o)
{
    if (o == 0u) return 255u;
    const uint64_t n = (uint64_t)z + o, v = (255u * (uint64_t)z + n / 2u) / n;
    return v < 1u ? 1u : v > 255u ? 255u : (uint32_t)v;
}

// entry i of the picture's table from its counts
FL_VP8_HD uint8_t vp8_ap_decide(uint32_t i, uint32_t z, uint32_t o)
{
    const uint32_t p_old = kVp8CoefProb[i], u = kVp8CoefUpdateProb[i], p_new = vp8_ap_candidate(z, o);
    if ((z | o) == 0u || p_new == p_old) return (uint8_t)p_old;
    const uint64_t with_new = (uint64_t)z * kVp8BitCost[p_new] + (uint64_t)o * kVp8BitCost[256u - p_new] + kVp8BitCost[256u - u] + 8u * 256u;
    const uint64_t with_old = (uint64_t)z * kVp8BitCost[p_old] + (uint64_t)o * kVp8BitCost[256u - p_old] + kVp8BitCost[u];
    return (uint8_t)(with_new < with_old ? p_new : p_old);
}

} // namespace fl
