// fl_vp8.hip -- the lossy WebP encoder on gfx950, so that what leaves the GPU for `webp=true` below quality 100 is the finished
// image/webp body (reference src/handler.rs:293-297, webp::Encoder::encode(q)) instead of the Y | U | V | A planes.  Opt-in
// (FLGPU_FE_WEBP_LOSSY and its variants: three switches, i4 / ap / lf, which fl_vp8_variant.h maps to front ends).  The stream is
// a VP8 key frame of this encoder's own choices -- it decodes to exactly the encoder's reconstruction, its bytes are not
// libwebp's; fl_vp8_core.h states the stream and holds all of its arithmetic, shared with the host twin (tests/vp8_host.cpp) and
// restated in tests/vp8_model.py.  This file is the choreography:
//   vp8_analyse_kernel  one wave per picture, macroblocks in raster order (a macroblock predicts from the reconstruction to its
//                       left and above).  Within a macroblock the work spreads over the lanes phase by phase: 495 loads, 96 block
//                       SSEs (4 modes x 24 blocks), 24 forward DCTs, 24 quantise / inverse DCT / reconstruct, 401 stores; the mode
//                       pick and the Y2 block are one lane's.  The macroblock lives in LDS, the reconstruction in scratch.
//   vp8_size_kernel     one lane per partition (partition 0 and up to 8 token partitions; 16 coder slots per picture, one lane in 16
//                       codes): the boolean coder runs without storing and leaves the partition's size.  The probability table is
//                       staged in LDS, a block's 16 levels are fetched whole.  The batch is the parallelism.
//   vp8_frame_kernel    one workgroup per picture: the layout from the sizes; RIFF / VP8X / ALPH / VP8 framing, the raw alpha
//                       plane where the planes kernel flagged a translucent pixel, the result word (0 if dst is too small).  With
//                       FLGPU_FEO_ALPHA_VP8L the alpha coder (fl_webpll.hip, alpha mode) has left the plane's VP8L stream: that goes
//                       into the chunk instead wherever it is strictly smaller (vp8_alph_size).
//   vp8_write_kernel    one lane per partition again: the same coder, storing at the partition's place in the file.
// i4 (fl_vp8_i4_core.h) has kernels of its own, so that the ones above stay as they are:
//   vp8_analyse_i4_kernel  the same walk; after the mode pick a macroblock whose I16 error exceeds the penalty tries its luma as
//                       sixteen sub-blocks, one after the other: 13 neighbour loads, 160 (mode, sample) errors over the 64 lanes
//                       in three rounds, each mode's sixteen summed across its lanes, then the chosen mode's residual through
//                       transform, quantiser and back on 16 lanes (4 for a transform pass).  The working copy and the trial's
//                       levels are in LDS; the winner of the two trials is committed.
//   vp8_size_kernel<true>, vp8_write_kernel<true>  the coder's instantiation with the mode tree in partition 0 and the type-3 / no-Y2
//                       path in the tokens, a branch per macroblock on its mode record.
// ap (fl_vp8_ap_core.h) shares the analysis kernels and adds one launch between the analysis and the size kernel:
//   vp8_stats_kernel<I4>  one workgroup per picture.  The (macroblock, block) pairs spread over its 256 threads; each fetches its
//                       block's levels whole, takes its contexts from the macroblock records and runs the coder's own token walk
//                       into a counting sink: 2 x 1056 counters in LDS (8448 B), LDS atomics.  After a barrier thread i < 1056
//                       applies the rule to entry i and stores the picture's table (1056 B of scratch).
//   vp8_size_kernel<I4, true>, vp8_write_kernel<I4, true>  the coders, staging the picture's table instead of the default one (a
//                       coder workgroup is exactly one picture) and writing the updates into partition 0.
// lf (fl_vp8_lf_core.h) shares all of the above and adds one launch in front of the first that codes partition 0 (the stats kernel
// where there is one, else the size kernel): the level's six bits move the boolean coder's state, so the sizes depend on it.
//   vp8_lf_kernel<I4>   one workgroup per (picture, candidate level).  Candidate 0 measures the reconstruction as it is.  The others
//                       copy it to a working copy of their own in scratch (the filter cascades in place; `rec` stays unfiltered for
//                       the coder's contexts) and run the decode front end's filter on it in vp8dec_filter_kernel's schedule:
//                       anti-diagonals d = x + 2 y, eight macroblocks of 32 lines a round, eight barrier-separated steps a
//                       macroblock -- which equals raster order.  Then all 256 threads sum the squared error over the visible
//                       samples in 64 bits and one thread stores the candidate's word.
//   vp8_size_kernel<I4, AP, true>, vp8_write_kernel<I4, AP, true>  the coders; the partition-0 lane derives the level from the
//                       picture's four words (vp8_lf_choice) and writes it into the frame header.
// FLGPU_FEO_SEGMENTS (fl_vp8_seg_core.h; a bit of flgpu_params::options on any of the front ends) adds one launch in front of
// everything, only when some job of the batch carries the option:
//   vp8_segment_kernel  one 256-thread workgroup per picture (it returns at once for a job without the option).  Waves stride over
//                       the macroblocks: 64 lanes x 4 luma samples, two wave reductions (mean, then activity), lane 0 stores the
//                       macroblock's bin and adds to a 256-word LDS histogram.  After a barrier the classification runs one
//                       thread per bin (class sums by LDS atomics, four threads move the centres), one thread derives the indices
//                       and the tree's probabilities and stores the picture's record, and all threads turn the stored bins into
//                       classes.  Batch-parallel, no chain between macroblocks.
// The analysis kernels then take each macroblock's steps from its class (vp8_seg_pick: one uniform branch and table look-up per
// macroblock), vp8_lf_inner dequantises a Y2 block with them, and the partition-0 lane of the coders writes the segment header and
// the ids (at run time, not a template axis).  Integer atomics only: the result does not depend on their order.
// A batch's pictures are grouped by front end in the job list, so each family (i4 | ap << 1 | lf << 2) is one range of it:
// launch_vp8_encode walks a table of the eight launch_family<I4, AP, LF> by that index.
// No kernel waits on another workgroup or wave, so there is no bounded wait and no use of the device error word.
// A lone large picture is latency-bound: one wave walks its macroblocks, nine lanes code it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_vp8.h"
#include "fl_vp8_ap_core.h"
#include "fl_vp8_i4_core.h"
#include "fl_vp8_lf_core.h"
#include "fl_vp8_seg_core.h"
#include "fl_wave.h"

namespace fl {
namespace {

constexpr uint32_t kLaneSlots = 16;    // coder slots per picture in the coder kernels: slot 0 = partition 0, 1..8 = token partitions
// Threads per coder slot, of which the first codes.  The coders' control flow is data, so lanes of one wave that code different
// partitions serialise each other's branches, and at one lane per slot the whole batch is 256 waves, one per CU.  Measured per
// batch of 1024 (profiles/pr_webp_lossy.txt): 1 -> 22.5 ms, 4 -> 21.4, 16 -> 19.2, 64 (a wave per coder) -> 29.7.
constexpr uint32_t kLaneStride = 16;
constexpr uint32_t kCoderThreads = 256;
constexpr uint32_t kFrameThreads = 256;
constexpr uint32_t kStatsThreads = 256;
constexpr uint32_t kLfThreads = 256;
constexpr uint32_t kSegThreads = 256;
static_assert(kSegThreads == kVp8SegBins, "the classification runs one thread per bin");
// the adaptive coders stage one table per workgroup: a workgroup's slots must be exactly one picture's
static_assert(kCoderThreads / kLaneStride == kLaneSlots && kCoderThreads % kLaneStride == 0, "a coder workgroup is one picture");

__device__ __forceinline__ Vp8Pic pic_of(const Vp8Job &j, const uint8_t *prob = kVp8CoefProb)
{
    Vp8Pic p;
    vp8_pic_dims(p, j.w, j.h);
    p.prob = prob;
    p.src = j.src; p.rec = j.rec; p.lev = j.lev; p.info = j.info; p.bm = j.bm;
    p.q = vp8_quant(j.qi);
    if (j.seg) { p.seg = reinterpret_cast<const Vp8SegRec *>(j.seg); p.segmap = j.seg + kVp8SegHead; } // (uniform over the picture)
    return p;
}

// The picture's classes and their quantiser indices (fl_vp8_seg_core.h states the rule).  Every barrier is in control flow uniform
// over the workgroup; no workgroup waits on another.
__global__ __launch_bounds__(kSegThreads) void vp8_segment_kernel(const Vp8Job *__restrict__ jobs)
{
    __shared__ uint32_t s_hist[kVp8SegBins];
    __shared__ uint32_t s_n[4], s_sum[4], s_lo, s_hi;
    __shared__ int32_t s_c[4];
    __shared__ uint8_t s_cls[kVp8SegBins];
    __shared__ Vp8SegRec s_rec;
    const Vp8Job &jb = jobs[blockIdx.x];
    if (!jb.seg) return; // (uniform) the job does not carry the option
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t mbw = vp8_mbs(jb.w), mbh = vp8_mbs(jb.h), mbs = mbw * mbh;
    uint8_t *map = jb.seg + kVp8SegHead;
    s_hist[tid] = 0u; s_cls[tid] = 0;
    if (tid < 4u) { s_n[tid] = 0u; s_sum[tid] = 0u; s_c[tid] = 0; }
    if (tid == 0u) { s_lo = kVp8SegBins; s_hi = 0u; }
    __syncthreads();
    // phase A: the activity of every macroblock; the bound is the wave's, all 64 lanes take part in both reductions
    for (uint32_t mb = wave; mb < mbs; mb += kSegThreads / 64u) {
        const uint32_t mbx = mb % mbw, mby = mb / mbw;
        uint32_t y[4], sum = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) { y[i] = vp8_seg_sample(jb.src, jb.w, jb.h, mbx, mby, lane * 4u + i); sum += y[i]; }
        const uint32_t m = vp8_seg_mean(wave_sum<uint32_t>(sum));
        uint32_t dev = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) dev += vp8_seg_dev(y[i], m);
        const uint32_t bin = vp8_seg_bin(wave_sum<uint32_t>(dev));
        if (lane == 0u) {
            map[mb] = (uint8_t)bin;
            atomicAdd(&s_hist[bin], 1u);
            if (bin) { atomicMin(&s_lo, bin); atomicMax(&s_hi, bin); }
        }
    }
    __syncthreads();
    // phase B: thread a is bin a
    const uint32_t lo = s_lo, hi = s_hi, mine = s_hist[tid];
    const bool ranged = lo < hi; // (uniform) else: no non-flat macroblock, or one occupied bin
    if (ranged) {
        if (tid < 4u) s_c[tid] = vp8_seg_centre0(lo, hi, tid);
        __syncthreads();
        for (uint32_t round = 0; round <= kVp8SegRounds; ++round) {
            if (tid >= lo && tid <= hi) {
                int32_t c[4] = {s_c[0], s_c[1], s_c[2], s_c[3]};
                const uint32_t k = vp8_seg_nearest((int32_t)tid, c);
                s_cls[tid] = (uint8_t)k;
                if (mine) { atomicAdd(&s_n[k], mine); atomicAdd(&s_sum[k], tid * mine); } // (below 2^32: 255 x the macroblock limit)
            }
            __syncthreads();
            if (round < kVp8SegRounds && tid < 4u) { s_c[tid] = vp8_seg_centre(s_sum[tid], s_n[tid], s_c[tid]); s_n[tid] = 0u; s_sum[tid] = 0u; }
            __syncthreads();
        }
    }
    if (tid == 0u) {
        const int32_t c[4] = {s_c[0], s_c[1], s_c[2], s_c[3]};
        const uint32_t n[4] = {s_n[0], s_n[1], s_n[2], s_n[3]};
        Vp8SegRec r;
        vp8_seg_finish(r, c, n, ranged ? s_hist[0] : 0u, jb.qi); // (not ranged: n = 0, not segmented)
        s_rec = r;
        *reinterpret_cast<Vp8SegRec *>(jb.seg) = r;
    }
    __syncthreads();
    // phase C: the bins become classes
    const bool on = s_rec.on != 0;
    for (uint32_t mb = tid; mb < mbs; mb += kSegThreads) map[mb] = on ? s_cls[map[mb]] : (uint8_t)0;
}

__global__ __launch_bounds__(64) void vp8_analyse_kernel(const Vp8Job *__restrict__ jobs)
{
    __shared__ Vp8Mb m;
    const Vp8Job &jb = jobs[blockIdx.x];
    Vp8Pic p = pic_of(jb);
    const uint32_t lane = threadIdx.x;
    for (uint32_t mby = 0; mby < p.mbh; ++mby)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) {
            vp8_seg_pick(p, (uint64_t)mby * p.mbw + mbx); // (uniform) FLGPU_FEO_SEGMENTS: the steps of the macroblock's class
            for (uint32_t k = lane; k < kVp8LoadItems; k += 64u) vp8_phase_load(p, m, mbx, mby, k);
            __syncthreads();
            if (lane < 3u) vp8_phase_dc(m, mbx, mby, lane);
            __syncthreads();
            for (uint32_t k = lane; k < kVp8SseItems; k += 64u) vp8_phase_sse(m, k);
            __syncthreads();
            if (lane == 0u) vp8_phase_modes(m);
            __syncthreads();
            if (lane < 24u) vp8_phase_fdct(m, lane);
            __syncthreads();
            if (lane == 0u) vp8_phase_y2(p, m);
            __syncthreads();
            if (lane < 24u) vp8_phase_recon(p, m, mbx, mby, lane);
            __syncthreads();
            for (uint32_t k = lane; k <= kVp8MbLevels; k += 64u) vp8_phase_store(p, m, mbx, mby, k);
            __syncthreads(); // the next macroblock overwrites m and reads this one's reconstruction
        }
}

// the I4 trial of one sub-block; every step's items are independent, a barrier separates the steps
__device__ __forceinline__ void i4_sub_block(const Vp8Pic &p, const Vp8Mb &m, Vp8I4 &t, uint32_t s, uint32_t lane)
{
    if (lane < kVp8I4EdgeItems) vp8_i4_phase_edges(m, t, s, lane);
    __syncthreads();
    // 160 items: lane l of round r has sample l % 16 of mode 4 r + l / 16, so a mode's sixteen errors sit in sixteen adjacent lanes
#pragma unroll
    for (uint32_t r = 0; r < 3u; ++r) {
        const uint32_t k = r * 64u + lane;
        uint32_t e = k < kVp8I4PredictItems ? vp8_i4_phase_predict(m, t, s, k) : 0u;
        e = group_sum<16>(e);
        if (k < kVp8I4PredictItems && (lane & 15u) == 0u) t.sse[k >> 4] = e;
    }
    __syncthreads();
    if (lane == 0u) vp8_i4_phase_pick(t, s);
    __syncthreads();
    if (lane < 16u) vp8_i4_phase_residual(m, t, s, lane);
    __syncthreads();
    if (lane < 4u) vp8_i4_phase_fdct_rows(t, lane);
    __syncthreads();
    if (lane < 4u) vp8_i4_phase_fdct_cols(t, lane);
    __syncthreads();
    if (lane < 16u) vp8_i4_phase_quant(p, t, s, lane);
    __syncthreads();
    if (lane < 4u) vp8_i4_phase_idct_cols(t, lane);
    __syncthreads();
    if (lane < 4u) vp8_i4_phase_idct_rows(t, lane);
    __syncthreads();
    if (lane < 16u) vp8_i4_phase_recon(t, s, lane);
    __syncthreads();
}

__global__ __launch_bounds__(64) void vp8_analyse_i4_kernel(const Vp8Job *__restrict__ jobs)
{
    __shared__ Vp8Mb m;
    __shared__ Vp8I4 t;
    const Vp8Job &jb = jobs[blockIdx.x];
    Vp8Pic p = pic_of(jb);
    const uint32_t lane = threadIdx.x;
    for (uint32_t mby = 0; mby < p.mbh; ++mby)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) {
            vp8_seg_pick(p, (uint64_t)mby * p.mbw + mbx); // (uniform) FLGPU_FEO_SEGMENTS: the steps of the macroblock's class
            for (uint32_t k = lane; k < kVp8LoadItems; k += 64u) vp8_phase_load(p, m, mbx, mby, k);
            if (lane < kVp8I4BeginItems) vp8_i4_phase_begin(p, t, mbx, mby, lane);
            __syncthreads();
            if (lane < 3u) vp8_phase_dc(m, mbx, mby, lane);
            __syncthreads();
            for (uint32_t k = lane; k < kVp8SseItems; k += 64u) vp8_phase_sse(m, k);
            __syncthreads();
            if (lane == 0u) vp8_phase_modes(m);
            __syncthreads();
            const uint32_t s16 = vp8_i4_s16(m); // (every lane: the decision is the wave's)
            bool i4 = false;
            if (vp8_i4_worth_trying(p, s16)) {
                for (uint32_t s = 0; s < 16u; ++s) i4_sub_block(p, m, t, s, lane);
                i4 = vp8_i4_wins(p, t, s16);
            }
            if (i4) {
                for (uint32_t k = lane; k < kVp8I4CommitItems; k += 64u) vp8_i4_phase_commit(p, m, t, mbx, mby, k);
                __syncthreads();
                if (lane < 8u) vp8_phase_fdct(m, 16u + lane);
                __syncthreads();
                if (lane < 8u) vp8_phase_recon(p, m, mbx, mby, 16u + lane);
            } else {
                if (lane < 24u) vp8_phase_fdct(m, lane);
                __syncthreads();
                if (lane == 0u) vp8_phase_y2(p, m);
                __syncthreads();
                if (lane < 24u) vp8_phase_recon(p, m, mbx, mby, lane);
            }
            __syncthreads();
            for (uint32_t k = lane; k < kVp8I4StoreItems; k += 64u) vp8_i4_phase_store(p, m, t, i4, mbx, mby, k);
            __syncthreads(); // the next macroblock overwrites m and t and reads this one's reconstruction and records
        }
}

// The counting sink of the token walk on the device: Vp8Count's counters in LDS, shared by the workgroup.
struct Vp8LdsCount {
    const uint8_t *tab;
    uint32_t *cnt;
    __device__ __forceinline__ void node(int bit, const uint8_t *p) { atomicAdd(cnt + (bit ? kVp8CoefProbs : 0u) + (uint32_t)(p - tab), 1u); }
    __device__ __forceinline__ void put(int, uint32_t) {}
};

// The picture's probability table from its token statistics.  No thread waits on another workgroup.
template <bool I4> __global__ __launch_bounds__(kStatsThreads) void vp8_stats_kernel(const Vp8Job *__restrict__ jobs)
{
    __shared__ uint32_t s_cnt[kVp8CountWords];
    const Vp8Job &jb = jobs[blockIdx.x];
    const Vp8Pic p = pic_of(jb); // (p.prob: the default table; the walk only takes addresses in it)
    for (uint32_t i = threadIdx.x; i < kVp8CountWords; i += kStatsThreads) s_cnt[i] = 0u;
    __syncthreads();
    Vp8LdsCount sink{p.prob, s_cnt};
    const uint32_t items = p.mbw * p.mbh * kVp8MbBlocks; // (under vp8_fits: below 2^20)
    for (uint32_t k = threadIdx.x; k < items; k += kStatsThreads) vp8_ap_count_item<I4>(sink, p, k);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kVp8CoefProbs; i += kStatsThreads) jb.tab[i] = vp8_ap_decide(i, s_cnt[i], s_cnt[kVp8CoefProbs + i]);
}

// the macroblock rows that have a macroblock on anti-diagonal d: y in [lo, lo + count), x = d - 2 y
__device__ __forceinline__ uint32_t lf_diagonal(const Vp8Pic &p, uint32_t d, uint32_t &lo)
{
    lo = d >= p.mbw ? (d - p.mbw + 2u) >> 1 : 0u;
    const uint32_t hi = min(p.mbh - 1u, d >> 1);
    return hi >= lo ? hi - lo + 1u : 0u;
}

// the level the loop-filtered coders write: a function of the picture's base level and its four cost words
__device__ __forceinline__ uint32_t lf_level_of(const Vp8Job &jb)
{
    const uint64_t *cost = reinterpret_cast<const uint64_t *>(jb.lf);
    const uint64_t D[kVp8LfCandidates] = {cost[0], cost[1], cost[2], cost[3]};
    return vp8_lf_choice(vp8_lf_base_of(jb.qi, jb.lf_base), D);
}

// One candidate level of one picture: filter a copy of the reconstruction as a decoder will, measure it against the source.
// Every barrier is in control flow uniform over the workgroup; no workgroup waits on another.
template <bool I4> __global__ __launch_bounds__(kLfThreads) void vp8_lf_kernel(const Vp8Job *__restrict__ jobs)
{
    __shared__ uint64_t s_sum[kLfThreads / 64u];
    const Vp8Job &jb = jobs[blockIdx.x / kVp8LfCandidates];
    const uint32_t cand = blockIdx.x % kVp8LfCandidates;
    const Vp8Pic p = pic_of(jb);
    const uint32_t base = vp8_lf_base_of(jb.qi, jb.lf_base);
    uint64_t *cost = reinterpret_cast<uint64_t *>(jb.lf);
    if (base == 0u) { if (threadIdx.x == 0u) cost[cand] = 0u; return; } // (uniform) nothing is evaluated
    const uint8_t *pix = p.rec;
    if (cand) { // (uniform)
        const uint64_t bytes = vp8_rec_bytes(p.mbw, p.mbh), pitch = (bytes + 255u) & ~(uint64_t)255u;
        uint8_t *copy = jb.lf + kVp8LfCostBytes + (cand - 1u) * pitch;
        // (384 bytes a macroblock, both buffers 256-byte aligned: whole 16-byte words)
        for (uint64_t i = threadIdx.x; i < bytes / 16u; i += kLfThreads) reinterpret_cast<uint4 *>(copy)[i] = reinterpret_cast<const uint4 *>(p.rec)[i];
        __syncthreads();
        const Vp8DecPic dp = vp8_lf_pic(p, copy);
        Vp8MbRecord r = vp8_lf_record<false>(p, 0u, vp8_lf_candidate(base, cand)); // the limits; `inner` per macroblock below
        const uint32_t slot = threadIdx.x / kVp8dFilterLanes, lane = threadIdx.x % kVp8dFilterLanes;
        constexpr uint32_t kSlots = kLfThreads / kVp8dFilterLanes;
        const uint32_t ndiag = p.mbw + 2u * (p.mbh - 1u);
        for (uint32_t d = 0; d < ndiag; ++d) {
            uint32_t lo;
            const uint32_t count = lf_diagonal(p, d, lo);
            for (uint32_t b0 = 0; b0 < count; b0 += kSlots) {
                const bool active = b0 + slot < count;
                const uint32_t mby = active ? lo + b0 + slot : 0u, mbx = active ? d - 2u * mby : 0u;
                r.inner = vp8_lf_inner<I4>(p, (uint64_t)mby * p.mbw + mbx);
                for (uint32_t s = 0; s < kVp8dFilterSteps; ++s) {
                    if (active) vp8d_filter(dp, r, mbx, mby, s, lane);
                    __syncthreads(); // the edges of a macroblock overlap, and the next diagonal reads what this one wrote
                }
            }
        }
        pix = copy;
    }
    uint64_t sum = 0;
    const uint32_t items = vp8_lf_items(p);
    for (uint32_t i = threadIdx.x; i < items; i += kLfThreads) sum += vp8_lf_sq_diff(p, pix, i);
    sum = wave_sum<unsigned long long>(sum);
    if ((threadIdx.x & 63u) == 0u) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint64_t t = 0;
        for (uint32_t k = 0; k < kLfThreads / 64u; ++k) t += s_sum[k];
        cost[cand] = t;
    }
}

// The coders read a probability for every boolean: the table's 1056 bytes go to LDS first (all threads of the workgroup, before
// any of them leaves).  AP: the table of the workgroup's picture.
template <bool AP> __device__ __forceinline__ void stage_prob(uint8_t *s_prob, const Vp8Job *jobs)
{
    const uint8_t *tab = AP ? jobs[blockIdx.x].tab : kVp8CoefProb;
    for (uint32_t i = threadIdx.x; i < sizeof(kVp8CoefProb); i += kCoderThreads) s_prob[i] = tab[i];
    __syncthreads();
}

// the partition of lane slot `part` (0 = the first partition), counted or written
template <bool I4, bool AP, bool LF> __device__ __forceinline__ void code_partition(Vp8Bool &bw, const Vp8Pic &p, const Vp8Job &jb, uint32_t part, uint32_t nparts)
{
    if (part == 0u) vp8_put_first_partition<I4, AP, LF>(bw, p, jb.qi, nparts, LF ? lf_level_of(jb) : 0u);
    else vp8_put_token_partition<I4>(bw, p, part - 1u, nparts);
}

template <bool I4, bool AP = false, bool LF = false> __global__ __launch_bounds__(kCoderThreads) void vp8_size_kernel(const Vp8Job *__restrict__ jobs, uint32_t njobs)
{
    __shared__ uint8_t s_prob[sizeof(kVp8CoefProb)];
    if (AP && blockIdx.x >= njobs) return; // (never: the grid is one workgroup per picture)
    stage_prob<AP>(s_prob, jobs);
    const uint32_t t = blockIdx.x * kCoderThreads + threadIdx.x, slot = t / kLaneStride, job = slot / kLaneSlots, part = slot % kLaneSlots;
    if (job >= njobs || t % kLaneStride) return;
    const Vp8Job &jb = jobs[job];
    const Vp8Pic p = pic_of(jb, s_prob);
    const uint32_t nparts = vp8_partitions(p.mbh);
    if (part >= kVp8SizeWords) return;
    if (part > nparts) { jb.sizes[part] = 0u; return; }
    Vp8Bool bw;
    code_partition<I4, AP, LF>(bw, p, jb, part, nparts);
    jb.sizes[part] = bw.pos;
}

// (the frame kernel and the coders both lay the file out: the rule for the ALPH payload is vp8_alph_size on the same words)
__device__ __forceinline__ Vp8Layout layout_of(const Vp8Job &jb, uint32_t nparts, uint32_t *size)
{
    for (uint32_t k = 0; k < 9u; ++k) size[k] = jb.sizes[k];
    const bool alpha = (jb.result[0] & 1u) != 0u;
    return vp8_layout(jb.w, jb.h, alpha, nparts, size, alpha && jb.alpha ? vp8_alph_size(jb.w, jb.h, jb.alpha[0]) : 0u);
}

__global__ __launch_bounds__(kFrameThreads) void vp8_frame_kernel(const Vp8Job *__restrict__ jobs)
{
    const Vp8Job &jb = jobs[blockIdx.x];
    const uint32_t nparts = vp8_partitions(vp8_mbs(jb.h));
    uint32_t size[9];
    const Vp8Layout L = layout_of(jb, nparts, size);
    const bool alpha = (jb.result[0] & 1u) != 0u;
    if (L.total > jb.dst_cap) { if (threadIdx.x == 0u) jb.result[1] = 0u; return; }
    if (threadIdx.x == 0u) {
        vp8_put_framing(jb.dst, L, jb.w, jb.h, alpha, nparts, size);
        jb.result[1] = L.total;
        if (jb.seg && reinterpret_cast<const Vp8SegRec *>(jb.seg)->on) jb.result[0] |= kVp8ResultSegments; // (this thread alone writes the word in this launch)
    }
    if (alpha) {
        const uint32_t npix = jb.w * jb.h;
        const bool vp8l = L.alph_size != 1u + npix; // (only with FLGPU_FEO_ALPHA_VP8L: the stream is strictly smaller than the plane)
        const uint8_t *a = vp8l ? reinterpret_cast<const uint8_t *>(jb.alpha) + kWebpllAlphaHead : jb.src + npix + 2u * ((jb.w + 1u) / 2u) * ((jb.h + 1u) / 2u);
        for (uint32_t i = threadIdx.x; i < L.alph_size - 1u; i += kFrameThreads) jb.dst[L.alph + 9u + i] = a[i];
        if (vp8l && threadIdx.x == 0u) jb.result[0] |= kVp8ResultAlphaVp8l; // (no other workgroup writes the word after the planes launch)
    }
}

template <bool I4, bool AP = false, bool LF = false> __global__ __launch_bounds__(kCoderThreads) void vp8_write_kernel(const Vp8Job *__restrict__ jobs, uint32_t njobs)
{
    __shared__ uint8_t s_prob[sizeof(kVp8CoefProb)];
    if (AP && blockIdx.x >= njobs) return; // (never: the grid is one workgroup per picture)
    stage_prob<AP>(s_prob, jobs);
    const uint32_t t = blockIdx.x * kCoderThreads + threadIdx.x, slot = t / kLaneStride, job = slot / kLaneSlots, part = slot % kLaneSlots;
    if (job >= njobs || t % kLaneStride) return;
    const Vp8Job &jb = jobs[job];
    const Vp8Pic p = pic_of(jb, s_prob);
    const uint32_t nparts = vp8_partitions(p.mbh);
    if (part > nparts) return;
    uint32_t size[9];
    const Vp8Layout L = layout_of(jb, nparts, size);
    if (L.total > jb.dst_cap) return; // vp8_frame_kernel has reported it
    Vp8Bool bw;
    bw.buf = jb.dst + L.part[part];
    code_partition<I4, AP, LF>(bw, p, jb, part, nparts);
}

} // namespace

template <bool I4, bool AP, bool LF> static hipError_t launch_family(const Vp8Job *jobs, uint32_t njobs, hipStream_t st)
{
    if (!njobs) return hipSuccess;
    const uint32_t coder_blocks = (uint32_t)(((uint64_t)njobs * kLaneSlots * kLaneStride + kCoderThreads - 1u) / kCoderThreads);
    if (I4) hipLaunchKernelGGL(vp8_analyse_i4_kernel, dim3(njobs), dim3(64), 0, st, jobs);
    else hipLaunchKernelGGL(vp8_analyse_kernel, dim3(njobs), dim3(64), 0, st, jobs);
    if (hipError_t e = hipGetLastError()) return e;
    if (LF) {
        hipLaunchKernelGGL(vp8_lf_kernel<I4>, dim3(njobs * kVp8LfCandidates), dim3(kLfThreads), 0, st, jobs);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (AP) {
        hipLaunchKernelGGL(vp8_stats_kernel<I4>, dim3(njobs), dim3(kStatsThreads), 0, st, jobs);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL((vp8_size_kernel<I4, AP, LF>), dim3(coder_blocks), dim3(kCoderThreads), 0, st, jobs, njobs);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vp8_frame_kernel, dim3(njobs), dim3(kFrameThreads), 0, st, jobs);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((vp8_write_kernel<I4, AP, LF>), dim3(coder_blocks), dim3(kCoderThreads), 0, st, jobs, njobs);
    return hipGetLastError();
}

hipError_t launch_vp8_encode(const Vp8Job *jobs, const uint32_t n[kVp8Families], hipStream_t st, uint32_t segmented)
{
    if (segmented) {
        uint32_t all = 0;
        for (uint32_t f = 0; f < kVp8Families; ++f) all += n[f];
        hipLaunchKernelGGL(vp8_segment_kernel, dim3(all), dim3(kSegThreads), 0, st, jobs);
        if (hipError_t e = hipGetLastError()) return e;
    }
    // family f = i4 | ap << 1 | lf << 2 (fl_vp8_variant.h vp8_family): one range of jobs after the other
    static hipError_t (*const family[kVp8Families])(const Vp8Job *, uint32_t, hipStream_t) = {
        launch_family<false, false, false>, launch_family<true, false, false>, launch_family<false, true, false>, launch_family<true, true, false>,
        launch_family<false, false, true>,  launch_family<true, false, true>,  launch_family<false, true, true>,  launch_family<true, true, true>};
    for (uint32_t f = 0; f < kVp8Families; ++f) {
        if (hipError_t e = family[f](jobs, n[f], st)) return e;
        jobs += n[f];
    }
    return hipSuccess;
}

} // namespace fl
