// fl_gifquant.hip -- FLGPU_ENCODE_GIF_QUANTIZE: a local table of at most 256 entries for every frame the palette kernel (fl_gif.hip)
// marked as above 256 colours.  The rule and its arithmetic are fl_gif_quant_core.h's; tests/gif_quant_model.py pins the bytes.
//
// Three launches behind the palette kernel, every one a workgroup (or a row of them) per frame that returns at once for an unmarked
// frame; nothing waits between workgroups, every barrier sits in control flow uniform over its workgroup, and the only atomics are
// integer additions, so no result depends on an order of arrival:
//   gif_cells_kernel   the precision s (an LDS hash of the reduced colours at s = 0, 1, 2, left as soon as it holds more than
//                      kGifQuantHashCells) and the cells' n and sums, added up in the frame's scratch at the hash slot (s = 3: at the
//                      15-bit cell number); 1,024 threads, each on a run of adjacent pixels
//   gif_split_kernel   the cells compacted into a list (in LDS up to kGifQuantHashCells cells), then the serial chain of at most 255
//                      splits: a step picks its box by a workgroup reduction over the cached choices, walks the list once (cells
//                      carry their box number), adds the upper half's sums in LDS and takes the lower one by subtraction; then
//                      entries, ranks, the frame's head and record
//   gif_qindex_kernel  the nearest entry of every opaque pixel: table in LDS, four pixels a thread, all lanes on one entry a step
// The palette kernel zeroed the cells' scratch of a marked frame; gif_index_kernel leaves marked frames alone.
#include <algorithm>

#include "fl_gif.h"
#include "fl_wave.h"

namespace fl {

namespace {

__device__ __forceinline__ uint32_t key_at(const uint8_t *frame, uint32_t p, uint32_t c)
{
    return c == 4u ? gq_key_rgba(reinterpret_cast<const uint32_t *>(frame)[p]) : gq_key_la(reinterpret_cast<const uint16_t *>(frame)[p]);
}
__device__ __forceinline__ uint32_t cell_slot(uint32_t reduced) { return (reduced * 0x9E3779B1u) >> 19; }
static_assert(kGifQuantHashSlots == 1u << 13, "cell_slot keeps 13 bits");
static_assert(kGifThreads == 256, "a thread per table entry and per box");
constexpr uint32_t kGqCellThreads = 1024;
static_assert(kGifQuantHashCells + kGqCellThreads < kGifQuantHashSlots, "the hash must hold the cells and one key per thread in flight");

// keys of pixels 4 q .. 4 q + 3; how many of them lie in the frame
__device__ __forceinline__ uint32_t load_quad(const uint8_t *frame, uint32_t q, uint32_t px, uint32_t c, uint32_t key[4])
{
    const uint32_t n = min(4u, px - 4u * q);
    if (c == 4u && n == 4u) {
        const uint4 v = reinterpret_cast<const uint4 *>(frame)[q];
        key[0] = gq_key_rgba(v.x); key[1] = gq_key_rgba(v.y); key[2] = gq_key_rgba(v.z); key[3] = gq_key_rgba(v.w);
    } else {
        for (uint32_t k = 0; k < n; ++k) key[k] = key_at(frame, 4u * q + k, c);
    }
    return n;
}

// A thread walks a run of adjacent pixels, four a load: a letterbox's bars and other flat areas fall to one thread as runs of one
// cell, which it adds up in registers; sixteen waves keep enough loads in flight for a walk that is all latency.
__global__ __launch_bounds__(kGqCellThreads) void gif_cells_kernel(GifEncJob J)
{
    __shared__ uint32_t s_tab[kGifQuantHashSlots];
    __shared__ uint32_t s_count, s_clear;
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    uint32_t *rec = J.frec + (size_t)f * kGifFrameRec;
    if (!rec[kGrQuant]) return;
    const uint8_t *frame = J.pixels + (size_t)f * J.pix_pitch;
    const uint32_t quads = (J.px + 3u) / 4u, per = (quads + kGqCellThreads - 1u) / kGqCellThreads;
    const uint32_t q0 = min(quads, tid * per), q1 = min(quads, q0 + per);
    if (tid == 0u) s_clear = 0u;
    volatile uint32_t *tab = s_tab;
    volatile uint32_t *count = &s_count;
    uint32_t s = 0u;
    for (; s < 3u; ++s) {
        for (uint32_t i = tid; i < kGifQuantHashSlots; i += kGqCellThreads) s_tab[i] = kGifQuantNoCell;
        if (tid == 0u) s_count = 0u;
        __syncthreads();
        uint32_t last = kGifQuantNoCell;
        bool full = false;
        for (uint32_t q = q0; q < q1 && !full; ++q) {
            uint32_t key[4];
            const uint32_t n = load_quad(frame, q, J.px, J.c, key);
            for (uint32_t k = 0; k < n; ++k) {
                if (*count > kGifQuantHashCells) { full = true; break; } // (at most kGifQuantHashCells + one per thread keys are ever in the table)
                if (!(key[k] & 255u)) continue;
                const uint32_t red = gq_reduced(key[k], s);
                if (red == last) continue;
                last = red;
                uint32_t h = cell_slot(red);
                for (uint32_t probe = 0; probe < kGifQuantHashSlots; ++probe, h = (h + 1u) & (kGifQuantHashSlots - 1u)) {
                    uint32_t cur = tab[h];
                    if (cur == kGifQuantNoCell) {
                        cur = atomicCAS(&s_tab[h], kGifQuantNoCell, red);
                        if (cur == kGifQuantNoCell) { atomicAdd(&s_count, 1u); break; }
                    }
                    if (cur == red) break;
                }
            }
        }
        __syncthreads();
        const uint32_t n = s_count;
        __syncthreads(); // (the next round resets the count)
        if (n <= kGifQuantHashCells) break;
    }
    // every opaque pixel into its cell
    uint32_t *qn = J.qcells + (size_t)f * 4u * J.qstride, *qr = qn + J.qstride, *qg = qr + J.qstride, *qb = qg + J.qstride;
    uint32_t last = kGifQuantNoCell, an = 0u, ar = 0u, ag = 0u, ab = 0u, clear = 0u;
    auto flush = [&] {
        if (!an) return;
        atomicAdd(&qn[last], an); atomicAdd(&qr[last], ar); atomicAdd(&qg[last], ag); atomicAdd(&qb[last], ab);
        an = ar = ag = ab = 0u;
    };
    for (uint32_t q = q0; q < q1; ++q) {
        uint32_t key[4];
        const uint32_t n = load_quad(frame, q, J.px, J.c, key);
        for (uint32_t k = 0; k < n; ++k) {
            if (!(key[k] & 255u)) { clear = 1u; continue; }
            uint32_t slot;
            if (s < 3u) {
                const uint32_t red = gq_reduced(key[k], s);
                slot = cell_slot(red); // (every reduced colour is in the table: the round that chose s ran to its end)
                for (uint32_t probe = 0; probe < kGifQuantHashSlots && s_tab[slot] != red; ++probe) slot = (slot + 1u) & (kGifQuantHashSlots - 1u);
            } else {
                slot = gq_cell15(key[k]);
            }
            if (slot != last) { flush(); last = slot; }
            an += 1u; ar += key[k] >> 24; ag += (key[k] >> 16) & 255u; ab += (key[k] >> 8) & 255u;
        }
    }
    flush();
    if (clear) atomicOr(&s_clear, 1u);
    __syncthreads();
    if (tid == 0u) rec[kGrQuant] = kGqMarked | s << kGqShift | (s_clear ? kGqClear : 0u);
}

// a thread's sums into the workgroup's (LDS; integers, so any order of arrival gives the same)
__device__ __forceinline__ void box_add_shared(GqBox *acc, const GqBox &v)
{
    if (!v.n) return;
    atomicAdd(&acc->n, v.n);
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicAdd(&acc->s[a], v.s[a]); atomicAdd(reinterpret_cast<unsigned long long *>(&acc->q[a]), (unsigned long long)v.q[a]); }
}

__global__ __launch_bounds__(kGifThreads) void gif_split_kernel(GifEncJob J)
{
    __shared__ GqBox s_box[256];
    __shared__ uint64_t s_word[256], s_max[kGifThreads / 64u]; // a box's (rank, number) for the selection; 0 = not splittable
    __shared__ uint32_t s_cut[256];                            // axis << 8 | cut
    __shared__ uint32_t s_sum[256][3], s_key[256], s_sorted[256];
    __shared__ uint32_t s_w[kGifThreads / 64u];
    __shared__ uint32_t s_n[kGifQuantHashCells], s_cb[kGifQuantHashCells]; // a list of at most kGifQuantHashCells cells: n, box << 24 | representative
    __shared__ GqBox s_up[2];                                               // the upper half's sums of this step and of the next
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    uint32_t *rec = J.frec + (size_t)f * kGifFrameRec;
    const uint32_t mark = rec[kGrQuant];
    if (!mark) return;
    const uint32_t s = (mark >> kGqShift) & 15u, clear = mark & kGqClear ? 1u : 0u, K = 256u - clear;
    uint32_t *qn = J.qcells + (size_t)f * 4u * J.qstride, *qr = qn + J.qstride, *qg = qr + J.qstride, *qb = qg + J.qstride;
    uint32_t *qbox = J.qbox + (size_t)f * J.qstride;
    s_sorted[tid] = 0u; s_sum[tid][0] = s_sum[tid][1] = s_sum[tid][2] = 0u; s_word[tid] = 0u;
    if (tid < 2u) gq_box_clear(s_up[tid]);
    // the cells in front of one another, in slot order (in place: a cell moves to a position at or in front of its slot, and the
    // scan's barriers stand between a round's reads and its writes)
    const uint32_t slots = s < 3u ? kGifQuantHashSlots : kGifQuantCells; // (s = 3 only with more than kGifQuantHashCells pixels: qstride covers it)
    uint32_t cells = 0u;
    GqBox mine;
    gq_box_clear(mine);
    for (uint32_t base = 0; base < slots; base += kGifThreads) {
        const uint32_t i = base + tid, n = qn[i], r = qr[i], g = qg[i], b = qb[i];
        uint32_t total;
        const uint32_t pos = cells + wg_scan<kGifThreads>(n ? 1u : 0u, s_w, &total);
        if (n) {
            const uint32_t c = gq_pack(gq_mean(r, n), gq_mean(g, n), gq_mean(b, n));
            qn[pos] = n; qr[pos] = r; qg[pos] = g; qb[pos] = b; qbox[pos] = c; // (box 0)
            if (pos < kGifQuantHashCells) { s_n[pos] = n; s_cb[pos] = c; }
            gq_box_add(mine, n, c);
        }
        cells += total;
    }
    box_add_shared(&s_up[1], mine); // (cleared in front of the scan's barriers; step 0 uses s_up[0] and clears this one again)
    __syncthreads();
    uint32_t boxes = cells ? 1u : 0u;
    auto settle = [&](uint32_t b) { // one thread: box b's choice from its statistics
        const GqChoice ch = gq_choice(s_box[b]);
        s_word[b] = gq_select_word(ch.rank, b);
        s_cut[b] = ch.axis << 8 | ch.cut;
    };
    if (tid == 0u && boxes) { s_box[0] = s_up[1]; settle(0u); }
    // the list in LDS where it fits (always at s < 3), else in the frame's scratch
    const bool lds = cells <= kGifQuantHashCells;
    uint32_t *cn = lds ? s_n : qn, *cb = lds ? s_cb : qbox;
    __syncthreads();
    for (uint32_t step = 0; boxes < K; ++step) {
        uint64_t word = wave_reduce(tid < boxes ? s_word[tid] : 0ull, [](uint64_t a, uint64_t b) { return a > b ? a : b; });
        if ((tid & 63u) == 0u) s_max[tid >> 6] = word;
        __syncthreads();
        word = 0u;
        for (uint32_t i = 0; i < kGifThreads / 64u; ++i) word = s_max[i] > word ? s_max[i] : word;
        if (!word) break; // (the same word in every thread)
        const uint32_t b = gq_selected_box(word), axis = s_cut[b] >> 8, cut = s_cut[b] & 255u;
        GqBox up;
        gq_box_clear(up);
        for (uint32_t i = tid; i < cells; i += kGifThreads) { // (cell i is always this thread's)
            const uint32_t w = cb[i];
            if ((w >> 24) == b && gq_axis_of(w, axis) > cut) {
                cb[i] = (w & 0x00ffffffu) | boxes << 24;
                gq_box_add(up, cn[i], w & 0x00ffffffu);
            }
        }
        GqBox *acc = &s_up[step & 1u];
        box_add_shared(acc, up); // (late boxes hold few cells: only the threads that moved one add anything)
        __syncthreads();
        // two threads of two waves settle the two boxes; the first also clears the sums of the step after this one
        if (tid == 0u) { gq_box_remove(s_box[b], *acc); settle(b); gq_box_clear(s_up[(step + 1u) & 1u]); }
        if (tid == 64u) { s_box[boxes] = *acc; settle(boxes); }
        ++boxes;
        __syncthreads();
    }
    // entries: the rounded means of the exact samples, ranked by (r, g, b, box number)
    for (uint32_t i = tid; i < cells; i += kGifThreads) {
        const uint32_t b = cb[i] >> 24;
        atomicAdd(&s_sum[b][0], qr[i]); atomicAdd(&s_sum[b][1], qg[i]); atomicAdd(&s_sum[b][2], qb[i]);
    }
    __syncthreads();
    if (tid < boxes) {
        const uint32_t N = s_box[tid].n;
        s_key[tid] = gq_pack(gq_mean(s_sum[tid][0], N), gq_mean(s_sum[tid][1], N), gq_mean(s_sum[tid][2], N)) << 8 | tid;
    }
    __syncthreads();
    if (tid < boxes) {
        const uint32_t key = s_key[tid];
        uint32_t rank = 0u;
        for (uint32_t j = 0; j < boxes; ++j) rank += s_key[j] < key ? 1u : 0u;
        s_sorted[rank] = key >> 8;
    }
    __syncthreads();
    const uint32_t n = boxes + clear; // (at least 1: a frame has a pixel)
    const uint32_t tbits = n <= 2u ? 1u : 32u - (uint32_t)__builtin_clz(n - 1u), tsize = 1u << tbits, mcs = tbits < 2u ? 2u : tbits;
    uint8_t *body = J.bodies + (size_t)f * J.body_pitch;
    if (tid < tsize) {
        const uint32_t k = s_sorted[tid]; // (zero beyond the boxes: the transparent entry and the padding)
        body[18u + 3u * tid] = (uint8_t)(k >> 16); body[19u + 3u * tid] = (uint8_t)(k >> 8); body[20u + 3u * tid] = (uint8_t)k;
        J.ckeys[(size_t)f * kGifColourSlots + tid] = k; // the table of gif_qindex_kernel
    }
    if (tid == 0u) {
        const uint32_t t = clear ? boxes : kGifNoTransparent;
        const uint8_t head[18] = {0x21, 0xf9, 4, (uint8_t)(clear ? 0x05 : 0x04), 0, 0, (uint8_t)(clear ? t : 0u), 0,
                                  0x2c, 0, 0, 0, 0, (uint8_t)J.w, (uint8_t)(J.w >> 8), (uint8_t)J.h, (uint8_t)(J.h >> 8), (uint8_t)(0x80u | (tbits - 1u))};
        for (uint32_t i = 0; i < 18u; ++i) body[i] = head[i];
        body[18u + 3u * tsize] = (uint8_t)mcs;
        rec[kGrColours] = n; rec[kGrTableBits] = tbits; rec[kGrCodeSize] = mcs; rec[kGrTransparent] = t;
        rec[kGrHeadBytes] = 19u + 3u * tsize;
        atomicAdd(&J.status[2], 1u);
    }
}

__global__ __launch_bounds__(kGifThreads) void gif_qindex_kernel(GifEncJob J)
{
    __shared__ uint32_t s_e[256];
    const uint32_t f = blockIdx.y, tid = threadIdx.x;
    const uint32_t *rec = J.frec + (size_t)f * kGifFrameRec;
    const uint32_t mark = rec[kGrQuant];
    if (!mark) return;
    const uint32_t boxes = rec[kGrColours] - (mark & kGqClear ? 1u : 0u);
    s_e[tid] = J.ckeys[(size_t)f * kGifColourSlots + tid]; // (beyond the table: whatever is there, never looked at)
    __syncthreads();
    const uint8_t *frame = J.pixels + (size_t)f * J.pix_pitch;
    uint32_t *out = reinterpret_cast<uint32_t *>(J.indices + (size_t)f * J.idx_pitch);
    const uint32_t quads = (J.px + 3u) / 4u;
    for (uint32_t q = blockIdx.x * kGifThreads + tid; q < quads; q += gridDim.x * kGifThreads) {
        uint32_t key[4] = {0u, 0u, 0u, 0u}; // (a pixel beyond the frame counts as clear; its byte lies in the pitch's slack)
        if (J.c == 4u && 4u * q + 4u <= J.px) {
            const uint4 v = reinterpret_cast<const uint4 *>(frame)[q];
            key[0] = gq_key_rgba(v.x); key[1] = gq_key_rgba(v.y); key[2] = gq_key_rgba(v.z); key[3] = gq_key_rgba(v.w);
        } else {
            for (uint32_t k = 0; k < 4u; ++k)
                if (4u * q + k < J.px) key[k] = key_at(frame, 4u * q + k, J.c);
        }
        uint32_t best[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, at[4] = {boxes, boxes, boxes, boxes};
        for (uint32_t i = 0; i < boxes; ++i) {
            const uint32_t e = s_e[i];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) gq_nearer(e, i, key[k], best[k], at[k]);
        }
        uint32_t word = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) word |= ((key[k] & 255u ? at[k] : boxes) & 255u) << (8u * k);
        out[q] = word;
    }
}

} // namespace

void launch_gif_quantize(const GifEncJob &J, hipStream_t st)
{
    const uint32_t quads = (J.px + 3u) / 4u;
    const uint32_t groups = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((quads + kGifThreads - 1) / kGifThreads, 1), 256);
    gif_cells_kernel<<<dim3(J.frames), dim3(kGqCellThreads), 0, st>>>(J);
    gif_split_kernel<<<dim3(J.frames), dim3(kGifThreads), 0, st>>>(J);
    gif_qindex_kernel<<<dim3(groups, J.frames), dim3(kGifThreads), 0, st>>>(J);
}

} // namespace fl
