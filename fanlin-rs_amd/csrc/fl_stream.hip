// fl_stream.hip -- the fused streaming Lanczos3 down-scale in f32 (S1_STREAM): what route_resample's try_stream (fl_batch.cpp) takes
// of the down-scales the matrix-pipe kernels (fl_mfma.hip, fl_wtile.hip) leave, pre-ops and unaligned Rgb8 rows included.
//
// resample_stream_kernel reads every source byte exactly once with coalesced 12/16-byte-per-lane buffer loads, keeps the <= 8
// live output rows of the vertical pass in registers (weights are wave-uniform SGPR operands of v_pk_fma_f32), hands finished
// f32 rows to the horizontal pass through LDS, and writes rounded u8 pixels straight into the (letterboxed) destination.
#include <atomic>

#include "fl_kernel_common.h"
#include "fl_kernels.h"

#ifndef FL_WPREFETCH
#define FL_WPREFETCH 0 // 1 = fetch a row's weights from LDS one row ahead (measured: no gain)
#endif

#ifndef FL_RING_MULT
#define FL_RING_MULT 2    // prefetch ring of the streaming kernel = FL_RING_MULT blocks of FL_STREAM_DEPTH rows
#endif
#ifndef FL_LOAD_AUX
#define FL_LOAD_AUX 0     // cache policy bits of the streaming kernel's source-row loads (experiments: 2 = nt)
#endif
#ifndef FL_STREAM_DEPTH
#define FL_STREAM_DEPTH 4 // source rows per block of the streaming kernel
#endif

namespace fl {

template <int CS> struct RowRaw;
template <> struct RowRaw<1> { uint32_t v; __device__ uint32_t dw(int) const { return v; } };
template <> struct RowRaw<2> { u32x2 v; __device__ uint32_t dw(int i) const { return i == 0 ? v.x : v.y; } };
template <> struct RowRaw<3> { u32x3 v; __device__ uint32_t dw(int i) const { return i == 0 ? v.x : i == 1 ? v.y : v.z; } };
template <> struct RowRaw<4> { u32x4 v; __device__ uint32_t dw(int i) const { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; } };

// Source-row loads are ordinary (compiler-counted) raw buffer loads.  What keeps them in flight across
// the horizontal pass is that the kernel's only global STORES (store_pixel_hidden) are issued from
// inline asm: on gfx9 loads and stores share vmcnt, and once hipcc sees a store inside the row loop it
// drains every outstanding load at the loop header (s_waitcnt vmcnt(0)), turning the D-deep prefetch
// ring into one exposed HBM round trip per block.  Hidden stores are safe: vector-memory operations
// retire in order, so a younger store the compiler does not know about can only make its counted
// waits longer, never shorter.
template <int CS>
__device__ __forceinline__ void load_row(RowRaw<CS> &r, __amdgpu_buffer_rsrc_t rs, uint32_t voff)
{
    if constexpr (CS == 1) r.v = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, FL_LOAD_AUX);
    if constexpr (CS == 2) r.v = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, 0, FL_LOAD_AUX);
    if constexpr (CS == 3) r.v = __builtin_amdgcn_raw_buffer_load_b96(rs, voff, 0, FL_LOAD_AUX);
    if constexpr (CS == 4) r.v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, FL_LOAD_AUX);
}

// PXL pixels of CS bytes, packed in CS dwords -> PXL*MC floats with the pre-op applied.
template <int CS, int PRE>
__device__ __forceinline__ void convert_row(const RowRaw<CS> &raw, float *v)
{
    constexpr int MC = mid_channels(CS, PRE);
    uint32_t d[CS];
#pragma unroll
    for (int k = 0; k < CS; ++k) d[k] = raw.dw(k);
    if (PRE == PRE_INVERT) {
        // 255 - c on every colour byte; alpha bytes (LumaA / Rgba) keep their value.
        constexpr uint32_t m = (CS == 2) ? 0x00ff00ffu : 0x00ffffffu; // bytes that are colour, per pixel-aligned dword
#pragma unroll
        for (int k = 0; k < CS; ++k) {
            if (CS == 2 || CS == 4) d[k] = d[k] ^ m; else d[k] = ~d[k];
        }
    }
    if (PRE == PRE_GRAY && CS >= 3) {
#pragma unroll
        for (int p = 0; p < PXL; ++p) {
            uint32_t s[CS];
#pragma unroll
            for (int c = 0; c < CS; ++c) {
                const int b = p * CS + c;
                s[c] = (d[b >> 2] >> (8 * (b & 3))) & 255u;
            }
            v[p * MC] = (float)luma_u8(s[0], s[1], s[2]);
            if (CS == 4) v[p * MC + 1] = (float)s[3];
        }
    } else {
#pragma unroll
        for (int b = 0; b < PXL * CS; ++b) v[b] = (float)((d[b >> 2] >> (8 * (b & 3))) & 255u); // v_cvt_f32_ubyteN
    }
}

// Takes the finished vertical row out of one accumulator slot (registers) and re-arms the slot.
template <int NH>
__device__ __forceinline__ void take_slot(f32x2 *acc, float *e)
{
#pragma unroll
    for (int j = 0; j < NH; ++j) { e[2 * j] = acc[j].x; e[2 * j + 1] = acc[j].y; acc[j] = f32x2{0.0f, 0.0f}; }
}

// NA = accumulator slots (output rows alive per source row; the host picks the smallest that fits),
// D  = source rows kept in flight per lane.
// UA (Rgb8 only): source rows that are not dword aligned (pitch or base pointer not a multiple of 4).  Dword
// buffer loads ignore the two low address bits, so each lane loads the 16 aligned bytes that cover its 12 and
// funnel-shifts them by the row's byte phase (v_alignbyte_b32; the phase is wave-uniform because a lane's
// own offset, 12 * lane, is a multiple of 4).
template <int CS, int PRE, bool LB, int NA, int D, bool UA>
__global__ __launch_bounds__(256) void resample_stream_kernel(const Job *__restrict__ jobs,
                                                              const StreamItem *__restrict__ items,
                                                              const uint32_t *__restrict__ arena
)
{
    // experiments only (-DFL_ABLATE=mask): 1 = no horizontal pass, 2 = no flush/barrier, 4 = no FMAs
#ifdef FL_ABLATE
    constexpr uint32_t ablate = FL_ABLATE;
#else
    constexpr uint32_t ablate = 0;
#endif
    constexpr int MC = mid_channels(CS, PRE);
    constexpr int NV = PXL * MC;
    constexpr uint32_t T = 256;
    float *lds = fl_lds;

    const StreamItem it = items[blockIdx.x];
    const Job jb = jobs[it.job];
    const uint32_t tid = threadIdx.x;
    const uint32_t nxs = it.x1 - it.x0;

    // LDS: [ sch: 2 x SCHED_CHUNK RowSched | WT: jmax x T float4 | PO: jmax x T u32 | pbuf: (nxs * ks + 1) x (float4, or float
    // for single-channel rows: the smaller buffer lets a third workgroup fit a CU) ]
    constexpr uint32_t SCH_WORDS = SCHED_CHUNK * (sizeof(RowSched) / 4);
    uint32_t *sch = reinterpret_cast<uint32_t *>(lds);
    const uint32_t jmax = it.jmax, kmax = it.kmax, ks = it.ks;
    f32x4 *wt = reinterpret_cast<f32x4 *>(lds + 2 * SCH_WORDS);
    uint32_t *po = reinterpret_cast<uint32_t *>(lds + 2 * SCH_WORDS + jmax * T * 4);
    const uint32_t pbuf_off = 2 * SCH_WORDS + jmax * T * 5; // float offset, a multiple of 4
    using PT = typename std::conditional<MC == 1, float, f32x4>::type; // one partial sum (all channels of one output column)
    PT *pbuf = reinterpret_cast<PT *>(lds + pbuf_off);

    // stage the strip's horizontal tables and zero the partial-sum buffer (slots no lane writes stay 0 forever)
    {
        const f32x4 *wsrc = reinterpret_cast<const f32x4 *>(arena + it.wt_off);
        for (uint32_t i = tid; i < jmax * T; i += T) { wt[i] = wsrc[i]; po[i] = arena[it.po_off + i]; }
        for (uint32_t i = tid; i < nxs * ks + 1; i += T) pbuf[i] = PT{};
        for (uint32_t i = tid; i < SCH_WORDS; i += T) sch[i] = arena[it.sched_off + i]; // first schedule chunk
    }

    // raw buffer descriptor (stride 0): num_records = image bytes, so the hardware range-checks every lane
    const uint32_t base_phase = UA ? (uint32_t)(reinterpret_cast<uintptr_t>(jb.src) & 3u) : 0u;
    // (UA: the range is rounded up to whole dwords, otherwise the hardware zeroes the last, partly valid dword;
    //  an aligned dword that holds one valid byte lies in the same page as that byte, so this cannot fault)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(jb.src) - base_phase, 0,
                                                                        (int)(UA ? ((jb.src_bytes + base_phase + 3u) & ~3u) : jb.src_bytes), 0x00020000);
    const uint32_t pitch = jb.sw * CS;
    const uint32_t voff = (it.sx0 + tid * PXL) * CS + it.r0 * pitch + base_phase;
    const uint32_t pix_base = (jb.oy - jb.cy) * jb.dw + jb.ox + (it.x0 - jb.cx);

    // Letterbox border: every workgroup paints the part of the fill frame that lies next to its own band
    // and strip (first/last band own the rows above/below the picture, first/last strip the side margins),
    // so no separate fill kernel runs over the destination.
    if (LB) {
        const uint32_t dx0 = it.x0 == jb.cx ? 0u : jb.ox + it.x0 - jb.cx;
        const uint32_t dx1 = it.x1 == jb.cx + jb.cw ? jb.dw : jb.ox + it.x1 - jb.cx;
        const uint32_t dy0 = it.y0 == jb.cy ? 0u : jb.oy + it.y0 - jb.cy;
        const uint32_t dy1 = it.y1 == jb.cy + jb.ch ? jb.dh : jb.oy + it.y1 - jb.cy;
        uint32_t *d32 = reinterpret_cast<uint32_t *>(jb.dst);
        // (hidden stores, like every store of this kernel: see load_row)
        // rows above and below the placed picture
        const uint32_t wcols = dx1 - dx0;
        const uint32_t top_rows = dy0 < jb.oy ? min(dy1, jb.oy) - dy0 : 0u;
        for (uint32_t i = tid; i < top_rows * wcols; i += T) store_hidden_b32(d32 + (dy0 + i / wcols) * jb.dw + dx0 + i % wcols, jb.fill);
        const uint32_t by0 = max(dy0, jb.oy + jb.ch);
        const uint32_t bot_rows = dy1 > by0 ? dy1 - by0 : 0u;
        for (uint32_t i = tid; i < bot_rows * wcols; i += T) store_hidden_b32(d32 + (by0 + i / wcols) * jb.dw + dx0 + i % wcols, jb.fill);
        // side margins of the rows that hold the picture
        const uint32_t my0 = max(dy0, jb.oy), my1 = min(dy1, jb.oy + jb.ch);
        const uint32_t mrows = my1 > my0 ? my1 - my0 : 0u;
        const uint32_t lcols = dx0 < jb.ox ? min(dx1, jb.ox) - dx0 : 0u;
        for (uint32_t i = tid; i < mrows * lcols; i += T) store_hidden_b32(d32 + (my0 + i / lcols) * jb.dw + dx0 + i % lcols, jb.fill);
        const uint32_t rx0 = max(dx0, jb.ox + jb.cw);
        const uint32_t rcols = dx1 > rx0 ? dx1 - rx0 : 0u;
        for (uint32_t i = tid; i < mrows * rcols; i += T) store_hidden_b32(d32 + (my0 + i / rcols) * jb.dw + rx0 + i % rcols, jb.fill);
    }

    // accumulators live as register PAIRS so that every tap is one v_pk_fma_f32 (two fused multiply-adds)
    static_assert(NV % 2 == 0, "PXL is even");
    constexpr int NH = NV / 2;
    f32x2 acc[NA][NH];
#pragma unroll
    for (int s = 0; s < NA; ++s)
#pragma unroll
        for (int k = 0; k < NH; ++k) acc[s][k] = f32x2{0.0f, 0.0f};

    // whole byte offset goes through voffset: rows past the image end are range-checked by the buffer descriptor and read 0
    constexpr int LW = UA ? 4 : CS; // dwords loaded per lane and row
    // rows in flight per lane: R.  HBM latency under load is longer than one block of FMAs, so the ring holds two blocks
    // where the register file allows it (Rgba8 accumulators and the unaligned variant's 4-dword rows already fill it)
    constexpr int RM = (!UA && CS <= 3) ? FL_RING_MULT : 1, R = D * RM;
    RowRaw<LW> ring[R];
#pragma unroll
    for (int k = 0; k < R; ++k) load_row<LW>(ring[k], rs, UA ? ((voff + k * pitch) & ~3u) : voff + k * pitch);

    __syncthreads();

    // Main loop: blocks of D source rows.  Inside a block the code is straight line (loads, byte->f32
    // conversion, one v_pk_fma_f32 per accumulator pair with the weight as an SGPR operand); rows that
    // complete an output row only record it, and the completed rows are flushed to LDS and run through
    // the horizontal pass between blocks.  The host guarantees that a completed slot is not re-armed
    // before the end of its block (build_row_sched, `defer` argument).
    // The row schedule (8 weights + live/emit masks per source row) is staged through LDS in chunks of
    // SCHED_CHUNK rows, double buffered: fetching it row by row with scalar loads exposes one scalar-cache
    // miss per row, which was the largest single stall of the loop.  The next chunk is fetched into two
    // VGPRs at the start of a chunk and written to the other LDS buffer at its end.
    const uint32_t nrows = it.r1 - it.r0; // the host pads the schedule to a whole number of chunks
    uint32_t g0 = 0, g1 = 0;
    // One block of D rows per pass of the inner loop; HALF selects which D registers of the ring the block consumes
    // and refills.  The inner loop is fully unrolled, so HALF is a constant and the ring stays in fixed registers.
    for (uint32_t rb0 = 0; rb0 < nrows; rb0 += R) { // nrows is a multiple of SCHED_CHUNK, hence of R
#pragma unroll
    for (int HALF = 0; HALF < RM; ++HALF) {
        const uint32_t rb = rb0 + HALF * D;
        const uint32_t in_chunk = rb % SCHED_CHUNK;
        const uint32_t *schc = sch + ((rb / SCHED_CHUNK) & 1u) * SCH_WORDS + in_chunk * (sizeof(RowSched) / 4);
        const bool fetch_next = in_chunk == 0 && rb + SCHED_CHUNK < nrows;
        if (fetch_next) {
            const uint32_t *nx = arena + it.sched_off + (size_t)(rb / SCHED_CHUNK + 1) * SCH_WORDS;
            g0 = nx[tid];
            if (tid + T < SCH_WORDS) g1 = nx[tid + T];
        }
        // block summary (row 0 of the block): which slots complete inside this block, first completed output row
        const u32x4 meta = *reinterpret_cast<const u32x4 *>(schc + 8);
        const uint32_t sch_base = (uint32_t)(schc - sch); // dword offset of this block's first row inside the dynamic LDS block
        // Row weights: wave-uniform LDS reads (broadcast), fetched ONE row ahead so that a row's FMAs never
        // wait for LDS.  Dead slots carry weight 0, so the accumulate below is branch free: acc + v * 0
        // leaves a finished or not yet started slot untouched, and skipping it with scalar branches costs
        // more than the idle v_pk_fma_f32 it saves.  (The opaque offsets stop hipcc from hoisting all D rows'
        // reads to the top of the block, which costs 8 VGPRs per row of look-ahead.)
        f32x4 wr03[D], wr47[D];
        {
            uint32_t so = sch_base;
            asm volatile("" : "+v"(so));
            wr03[0] = *reinterpret_cast<const f32x4 *>(fl_lds + so);
            wr47[0] = *reinterpret_cast<const f32x4 *>(fl_lds + so + 4);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const uint32_t ri = rb + k;
            if (k + 1 < D && FL_WPREFETCH) {
                uint32_t so = sch_base + (k + 1) * 12;
                asm volatile("" : "+v"(so));
                wr03[k + 1 < D ? k + 1 : 0] = *reinterpret_cast<const f32x4 *>(fl_lds + so);
                wr47[k + 1 < D ? k + 1 : 0] = *reinterpret_cast<const f32x4 *>(fl_lds + so + 4);
            }
            if (k > 0 && !FL_WPREFETCH) {
                uint32_t so = sch_base + k * 12;
                asm volatile("" : "+v"(so));
                wr03[k] = *reinterpret_cast<const f32x4 *>(fl_lds + so);
                wr47[k] = *reinterpret_cast<const f32x4 *>(fl_lds + so + 4);
            }
            const f32x4 w03 = wr03[k], w47 = wr47[k];
            // unconditional refill: rows past the band are harmless extra reads, rows past the image read 0
            // (convert first, refill second: the slot's registers are dead by then, so the refill lands in place)
            float v[NV];
            if constexpr (UA) {
                const uint32_t ph = __builtin_amdgcn_readfirstlane((voff + ri * pitch) & 3u); // same in every lane
                RowRaw<CS> al;
                al.v.x = __builtin_amdgcn_alignbyte(ring[HALF * D + k].v.y, ring[HALF * D + k].v.x, ph);
                al.v.y = __builtin_amdgcn_alignbyte(ring[HALF * D + k].v.z, ring[HALF * D + k].v.y, ph);
                al.v.z = __builtin_amdgcn_alignbyte(ring[HALF * D + k].v.w, ring[HALF * D + k].v.z, ph);
                convert_row<CS, PRE>(al, v);
            } else {
                convert_row<CS, PRE>(ring[HALF * D + k], v); // hipcc waits for this row only: the R - 1 younger rows stay in flight
            }
            // Keep the refill below the conversion: hoisted above it, the refill needs fresh registers and the
            // ring is then rotated with v_mov behind a vmcnt(0) at the loop end.  The empty asm makes the
            // refill's address depend on every converted value, so all reads of the old row precede it.
            uint32_t roff = voff + (ri + R) * pitch;
#pragma unroll
            for (int j = 0; j < NV; ++j) asm volatile("" : "+v"(roff) : "v"(v[j]));
            load_row<LW>(ring[HALF * D + k], rs, UA ? (roff & ~3u) : roff);
            if (!(ablate & 4u)) {
#pragma unroll
                for (int s = 0; s < NA; ++s) {
                    const float w = s == 0 ? w03.x : s == 1 ? w03.y : s == 2 ? w03.z : s == 3 ? w03.w
                                  : s == 4 ? w47.x : s == 5 ? w47.y : s == 6 ? w47.z : w47.w;
                    const f32x2 ww = {w, w};
#pragma unroll
                    for (int j = 0; j < NH; ++j)
                        acc[s][j] = __builtin_elementwise_fma(f32x2{v[2 * j], v[2 * j + 1]}, ww, acc[s][j]);
                }
            }
            // One row at a time: left alone, hipcc converts all D rows and reads all D weight sets up front
            // and sinks every FMA to the end of the block, which costs 20 VGPRs per row of look-ahead (and a
            // wave per SIMD).  The empty asm pins each accumulator's value here, the barrier pins the rest.
#pragma unroll
            for (int s = 0; s < NA; ++s)
#pragma unroll
                for (int j = 0; j < NH; ++j) asm volatile("" : "+v"(acc[s][j])); // pinned as pairs: keeps v_pk_fma_f32
            __builtin_amdgcn_sched_barrier(0);
        }
        uint32_t em = __builtin_amdgcn_readfirstlane(meta.y); // outputs complete in order: first_out, first_out + 1, ...
        uint32_t oy = __builtin_amdgcn_readfirstlane(meta.z);
        // g0/g1 were loaded by the compiler's own bookkeeping; publish the next chunk before its first use
        if (in_chunk + D == SCHED_CHUNK && rb + D < nrows) {
            uint32_t *nb = sch + (((rb / SCHED_CHUNK) + 1) & 1u) * SCH_WORDS;
            nb[tid] = g0;
            if (tid + T < SCH_WORDS) nb[tid + T] = g1;
            lds_barrier();
        }
        if (ablate & 2u) em = 0;
        while (em) { // wave-uniform; usually zero or one iteration
            const uint32_t s = oy % NA;
            em &= ~(1u << s);
            float e[NV]; // the finished f32 row: this lane's PXL pixels x MC channels
            switch (s) {
            case 0: take_slot<NH>(acc[0], e); break;
            case 1: take_slot<NH>(acc[NA > 1 ? 1 : 0], e); break;
            case 2: take_slot<NH>(acc[NA > 2 ? 2 : 0], e); break;
            case 3: take_slot<NH>(acc[NA > 3 ? 3 : 0], e); break;
            case 4: take_slot<NH>(acc[NA > 4 ? 4 : 0], e); break;
            case 5: take_slot<NH>(acc[NA > 5 ? 5 : 0], e); break;
            case 6: take_slot<NH>(acc[NA > 6 ? 6 : 0], e); break;
            default: take_slot<NH>(acc[NA > 7 ? 7 : 0], e); break;
            }
            if (!(ablate & 1u) && !(ablate & 16u)) {
                // Horizontal pass, step 1 (all lanes): this lane's 4 pixels -> one partial sum per output
                // column whose window they touch.  Weights and target slots come from per-lane tables, so
                // every LDS access is lane-contiguous (no bank conflicts).
#pragma unroll 4
                for (uint32_t j = 0; j < jmax; ++j) { // jmax is a multiple of 4 (host pads with zero weights -> dummy slot)
                    const f32x4 w = wt[j * T + tid];
                    const uint32_t slot = po[j * T + tid];
                    float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int p = 0; p < PXL; ++p) {
                        const float wp = p == 0 ? w.x : p == 1 ? w.y : p == 2 ? w.z : w.w;
#pragma unroll
                        for (int c = 0; c < MC; ++c) part[c] = __builtin_fmaf(e[p * MC + c], wp, part[c]);
                    }
                    if constexpr (MC == 1) {
                        *reinterpret_cast<float *>(reinterpret_cast<char *>(pbuf) + (slot >> 2)) = part[0]; // table offsets are in 16-byte slots
                    } else {
                        f32x4 q;
                        q.x = part[0]; q.y = part[1]; q.z = part[2]; q.w = part[3];
                        *reinterpret_cast<f32x4 *>(reinterpret_cast<char *>(pbuf) + slot) = q;
                    }
                }
            }
            // LDS-only hand-off (no vmcnt drain: the prefetched rows and the pixel stores stay in flight)
            if (!(ablate & 8u)) lds_barrier();
            // step 2 (one lane per output column): add the partial sums in ascending pixel order.  The partial
            // sums are fetched into registers first and the second barrier sits right behind the fetch, so
            // the other waves go back to the vertical pass while the additions, rounding and store run.
            // partial sums held in registers across the barrier; Rgba8 rows (16 accumulators per slot) cannot afford 12 x 4
            constexpr uint32_t KREG = (MC == 4) ? 2 : 12;
            PT q[KREG];
            const PT *pp = pbuf + tid * ks;
            const bool reducer = !(ablate & 1u) && !(ablate & 32u) && tid < nxs;
            if (reducer) {
#pragma unroll
                for (uint32_t k = 0; k < KREG; ++k) q[k] = k < kmax ? pp[k] : PT{};
            }
            float sum[MC];
#pragma unroll
            for (int c = 0; c < MC; ++c) sum[c] = 0.0f;
            auto add_partial = [&](const PT &r) {
                if constexpr (MC == 1) sum[0] = sum[0] + r;
                else {
                    sum[0] = sum[0] + r.x;
                    if constexpr (MC > 1) sum[1] = sum[1] + r.y;
                    if constexpr (MC > 2) sum[2] = sum[2] + r.z;
                    if constexpr (MC > 3) sum[3] = sum[3] + r.w;
                }
            };
            if (reducer && kmax > KREG) { // long windows (ratio > ~7): finish the fetch before releasing the buffer
#pragma unroll
                for (uint32_t k = 0; k < KREG; ++k) add_partial(q[k]);
                for (uint32_t k = KREG; k < kmax; ++k) add_partial(pp[k]);
            }
            if (!(ablate & 8u)) lds_barrier();
            if (reducer) {
                if (kmax <= KREG) {
#pragma unroll
                    for (uint32_t k = 0; k < KREG; ++k) add_partial(q[k]); // slots past kmax hold +0: adding them changes nothing
                }
                uint32_t c8[MC];
#pragma unroll
                for (int c = 0; c < MC; ++c) c8[c] = round_u8(sum[c]);
                store_pixel<MC, LB, true>(jb.dst, pix_base + oy * jb.dw + tid, c8, jb.fill);
            }
            ++oy;
        }
    }
    }
}

// host-side sizing and the launch wrapper (called from the host runtime; asynchronous on `st`)

size_t stream_lds_bytes(uint32_t jmax, uint32_t nxs, uint32_t ks, uint32_t mid_channels)
{
    const size_t pbuf = (((size_t)nxs * ks + 1) * (mid_channels == 1 ? 4 : 16) + 15) & ~(size_t)15;
    return 2 * SCHED_CHUNK * sizeof(RowSched) + (size_t)jmax * 256 * 20 + pbuf;
}

uint32_t stream_lanes() { return 256; }

uint32_t stream_block_rows() { return FL_STREAM_DEPTH; }
static_assert(SCHED_CHUNK % (FL_STREAM_DEPTH * FL_RING_MULT) == 0 && FL_RING_MULT >= 1 && FL_RING_MULT <= 2, "schedule chunks must hold whole ring rounds");

bool stream_supported(uint32_t cs, uint32_t pre)
{
    (void)pre;
    return cs >= 1 && cs <= 4;
}

template <int CS, int PRE, bool LB, int NA, int D, bool UA>
static hipError_t launch_stream_v(const LaunchStream &s, hipStream_t st)
{
    // Ceiling of the kernel's dynamic LDS: get_stream_plan (fl_context.cpp) rejects a plan whose stream_lds_bytes() exceed it, and
    // s.lds_bytes is the maximum over the plans of the launch's pictures.
    constexpr size_t kStreamLdsMax = 150 * 1024;
    auto k = resample_stream_kernel<CS, PRE, LB, NA, D, UA>;
    static std::atomic<uint64_t> attr_set{0}; // the attribute is per function and device: set once per (instantiation, device)
    if (s.lds_bytes > kStreamLdsMax) return hipErrorInvalidValue;
    if (hipError_t e = set_max_lds_once(attr_set, (int)kStreamLdsMax, {reinterpret_cast<const void *>(k)}); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(s.nitems), dim3(256), s.lds_bytes, st, s.jobs, s.items, s.arena);
    return hipGetLastError();
}

hipError_t launch_stream(const LaunchStream &s, hipStream_t st)
{
    return dispatch_cs_pre(s.cs, s.pre, [&](auto cs, auto pre) {
        return dispatch_bool(s.letterbox, [&](auto lb) { return dispatch_bool(s.nacc <= 7, [&](auto seven) {
            constexpr int CS = decltype(cs)::value, PRE = decltype(pre)::value, NA = decltype(seven)::value ? 7 : 8, D = FL_STREAM_DEPTH;
            constexpr bool LB = decltype(lb)::value;
            if constexpr (CS == 3) if (s.unaligned) return launch_stream_v<CS, PRE, LB, NA, D, true>(s, st); // (the funnel-shift variant exists for Rgb8 only)
            return launch_stream_v<CS, PRE, LB, NA, D, false>(s, st);
        }); });
    });
}

} // namespace fl
