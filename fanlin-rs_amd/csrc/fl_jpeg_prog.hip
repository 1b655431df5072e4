// fl_jpeg_prog.hip -- FLGPU_FEO_JPEG_PROGRESSIVE on gfx950: the JPEG encoder of fl_jpeg.hip writing a progressive file (SOF2) of five
// scans by spectral selection; fl_jpeg_prog_core.h states the file and the rules.  Four kernels per batch behind one clear of the
// counts: jpeg_prog_stats_kernel (the transform phase of jpeg_dct_quant_kernel; every band's symbols counted in LDS, the DC terms and
// each band's flags left per block), jpeg_prog_tables_kernel (one workgroup per picture: which block carries which end-of-band run,
// the DC counts, the rule of fl_jpeg_opt_core.h six times, the five scans' headers), jpeg_prog_code_kernel (the transform again; a
// lane codes its unit's band -- the Y lanes two -- and the run its block carries into one 16-byte record per AC scan and block) and
// jpeg_prog_pack_kernel (one workgroup per picture, scan after scan: header, bit offsets, assembly in the LDS window, padding,
// stuffing).  A translation unit of its own: the modules of the other JPEG encode kernels hold what they held.
#include "fl_jpeg_dev.h"
#include "fl_jpeg_prog_core.h"

namespace fl {

namespace {

static_assert(kBlocksPerWave == 16u, "lanes 16 k + b hold component k of block b");
constexpr uint32_t kProgThreads = 256;   // jpeg_prog_tables_kernel: thread s is symbol s of each table, and block c + s of a step over the blocks
constexpr uint32_t kProgWaves = kProgThreads / 64u;
// a record's longest code: the band's coefficients and one run code -- no run code behind a non-zero coefficient 63
static_assert(62u * (16u + 10u) + 16u + 14u <= kAcWordsPerUnit * 32u && 63u * (16u + 10u) <= kAcWordsPerUnit * 32u, "a record's code must fit its acbits slot");

__device__ __forceinline__ uint16_t *prog_runs(uint32_t *rec, uint32_t nblocks)
{
    return reinterpret_cast<uint16_t *>(rec + kJpegProgHeadWords) + (size_t)nblocks * 3u;
}

// ---------------------------------------------------------------- kernel 1: statistics --

// Counts the symbols of AC scan k of one unit (cf, its mask m) into h and leaves the band's flags.
__device__ __forceinline__ void count_band(uint32_t *h, const int16_t *cf, uint64_t m, uint32_t k, uint16_t *flags)
{
    const JpegProgBand band = jpeg_prog_band(k);
    uint64_t bm = m & jpeg_prog_band_mask(band.ss, band.se);
    uint32_t prev = band.ss - 1u;
    while (bm) {
        const uint32_t pos = (uint32_t)__builtin_ctzll(bm);
        bm &= bm - 1ull;
        const int32_t cv = cf[pos];
        uint32_t run = pos - prev - 1u;
        prev = pos;
        while (run > 15u) { atomicAdd(&h[0xF0], 1u); run -= 16u; }
        const uint32_t mag = (uint32_t)(cv < 0 ? -cv : cv);
        atomicAdd(&h[(run << 4) | (32u - (uint32_t)__clz(mag))], 1u);
    }
    *flags = (uint16_t)jpeg_prog_flags(m, band.ss, band.se);
}

// The grid and the transform phase of jpeg_dct_quant_kernel.  Lane 16 k + b walks the mask of component k of block b once per band
// it has (Y: 1-5 and 6-63) and counts the band's symbols in the workgroup's LDS histograms, one per AC scan; the end-of-band runs
// span blocks, waves and workgroups, so they are counted by jpeg_prog_tables_kernel from the flags left here.
__global__ __launch_bounds__(kJpegThreads) void jpeg_prog_stats_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                       uint32_t job_base, uint32_t *__restrict__ prog, uint32_t *__restrict__ hist)
{
    __shared__ WaveLds s_w[kWavesPerWg];
    __shared__ uint32_t s_hist[kJpegProgHistWords];
    const JpegJob jb = jobs[job_base + blockIdx.y];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t nblocks = jb.bx * jb.by;
    if (blockIdx.x * kBlocksPerWg >= nblocks) return;    // whole workgroup idle (uniform)
    for (uint32_t i = threadIdx.x; i < kJpegProgHistWords; i += kJpegThreads) s_hist[i] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * kBlocksPerWg + wave * kBlocksPerWave;
    if (first < nblocks) {                               // (wave-uniform; every wave reaches the barrier below)
        const uint32_t count = min(kBlocksPerWave, nblocks - first);
        WaveLds &w = s_w[wave];
        if (jb.c == 4u && (reinterpret_cast<uintptr_t>(jb.src) & 3u) == 0u) transform_blocks<true>(jb, arena, first, count, lane, w);
        else transform_blocks<false>(jb, arena, first, count, lane, w);
        wave_lds_sync();
        const uint32_t b = lane & 15u, comp = lane >> 4;
        if (comp < 3u && b < count) {
            uint32_t *rec = prog + jb.opt_off;
            int16_t *dcs = reinterpret_cast<int16_t *>(rec + kJpegProgHeadWords);
            uint16_t *runs = prog_runs(rec, nblocks);
            const uint32_t u = b * 3u + comp, blk = first + b;
            const int16_t *cf = w.coef[u];
            const uint64_t m = w.nz[u];
            dcs[blk * 3u + comp] = cf[0];
            count_band(s_hist + 256u * comp, cf, m, comp, runs + (size_t)comp * nblocks + blk);
            if (comp == 0u) count_band(s_hist + 256u * 3u, cf, m, 3u, runs + (size_t)3u * nblocks + blk);
        }
    }
    __syncthreads();
    uint32_t *g = hist + (size_t)blockIdx.y * kJpegProgHistWords;
    for (uint32_t i = threadIdx.x; i < kJpegProgHistWords; i += kJpegThreads) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&g[i], v);
    }
}

// ---------------------------------------------------------------- kernel 2: runs, tables, headers --

// The greatest set bit below position i / the least set bit above position i of a kProgThreads-bit mask (-1 / kProgThreads: none)
__device__ __forceinline__ int32_t mask_prev(const uint64_t *m, uint32_t i)
{
    for (int32_t w = (int32_t)(i >> 6); w >= 0; --w) {
        const uint64_t v = w == (int32_t)(i >> 6) ? m[w] & ((1ull << (i & 63u)) - 1ull) : m[w];
        if (v) return w * 64 + 63 - (int32_t)__builtin_clzll(v);
    }
    return -1;
}
__device__ __forceinline__ uint32_t mask_next(const uint64_t *m, uint32_t i)
{
    for (uint32_t w = i >> 6; w < kProgWaves; ++w) {
        const uint64_t v = w == (i >> 6) ? m[w] & ~((2ull << (i & 63u)) - 1ull) : m[w];
        if (v) return w * 64u + (uint32_t)__builtin_ctzll(v);
    }
    return kProgThreads;
}

__device__ __forceinline__ int32_t mask_last(const uint64_t *m)
{
    for (int32_t w = (int32_t)kProgWaves - 1; w >= 0; --w)
        if (m[w]) return w * 64 + 63 - (int32_t)__builtin_clzll(m[w]);
    return -1;
}
__device__ __forceinline__ uint32_t mask_first(const uint64_t *m)
{
    for (uint32_t w = 0; w < kProgWaves; ++w)
        if (m[w]) return w * 64u + (uint32_t)__builtin_ctzll(m[w]);
    return kProgThreads;
}

// One workgroup per picture.  For each AC scan, two walks over the blocks' flags, kProgThreads blocks a step, thread s always block
// c + s: forwards with the last block that holds a coefficient (and whether its band ends in a zero) carried from step to step --
// which blocks carry a run code (jpeg_prog_run_head; every 32,767th block of a run) --, backwards with the next such block carried
// -- how long that run is (jpeg_prog_run_of); the run codes are counted into the scan's histogram.  Then the DC histograms from the
// DC terms and the rule of fl_jpeg_opt_core.h for the six tables as jpeg_opt_tables_kernel runs it: ranks and places in parallel,
// the serial part on one thread per table, tables t and t + 4 on wave t.  Out: the picture's record (fl_jpeg.h).
__global__ __launch_bounds__(kProgThreads) void jpeg_prog_tables_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                        uint32_t job_base, uint32_t *__restrict__ prog, const uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_cnt[kJpegProgTables][256];
    __shared__ uint32_t s_A[kJpegProgTables][kJpegOptMaxLeaves + 1u];
    __shared__ JpegOptCode s_code[kJpegProgTables];
    __shared__ uint8_t s_len[kJpegProgTables][256], s_vals[kJpegProgTables][256];
    __shared__ uint32_t s_used[kJpegProgTables];
    __shared__ uint64_t s_busy[kProgWaves], s_tail[kProgWaves];
    const JpegJob jb = jobs[job_base + blockIdx.x];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, nblocks = jb.bx * jb.by, nunits = nblocks * 3u;
    uint32_t *rec = prog + jb.opt_off;
    const uint32_t *g = hist + (size_t)blockIdx.x * kJpegProgHistWords;
    s_cnt[0][tid] = 0u; s_cnt[1][tid] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kJpegProgAcScans; ++k) s_cnt[2u + k][tid] = g[256u * k + tid];
    __syncthreads();

    // ---- the runs ----
    for (uint32_t k = 0; k < kJpegProgAcScans; ++k) {
        uint16_t *runs = prog_runs(rec, nblocks) + (size_t)k * nblocks;
        int64_t prev = -1;                                // (uniform) the last block of the steps so far that holds a coefficient
        bool prev_tail = false;
        for (uint32_t c0 = 0; c0 < nblocks; c0 += kProgThreads) {
            const uint32_t b = c0 + tid;
            const uint32_t bf = b < nblocks ? runs[b] : kJpegProgEmpty;
            const bool busy = !(bf & kJpegProgEmpty), tail = (bf & kJpegProgTail) != 0u;
            const uint64_t mb = __ballot(busy), mt = __ballot(tail);
            if ((tid & 63u) == 0u) { s_busy[wave] = mb; s_tail[wave] = mt; }
            __syncthreads();
            const int32_t p = mask_prev(s_busy, tid);
            const uint32_t head = busy ? b : p >= 0 ? jpeg_prog_run_head((int64_t)c0 + p, (s_tail[p >> 6] >> (p & 63)) & 1ull) : jpeg_prog_run_head(prev, prev_tail);
            if (b < nblocks) runs[b] = (uint16_t)(bf | ((tail && (b - head) % kJpegProgEobLimit == 0u) ? 4u : 0u));
            const int32_t last = mask_last(s_busy);
            if (last >= 0) { prev = (int64_t)c0 + last; prev_tail = (s_tail[last >> 6] >> (last & 63)) & 1ull; }
            __syncthreads();
        }
        uint32_t next = nblocks;                          // (uniform) the first block of the steps so far that holds a coefficient
        for (uint32_t c0 = (nblocks - 1u) / kProgThreads * kProgThreads;; c0 -= kProgThreads) {
            const uint32_t b = c0 + tid;
            const uint32_t bf = b < nblocks ? runs[b] : kJpegProgEmpty;
            const uint64_t mb = __ballot(!(bf & kJpegProgEmpty));
            if ((tid & 63u) == 0u) s_busy[wave] = mb;
            __syncthreads();
            const uint32_t n = mask_next(s_busy, tid);
            if (b < nblocks) {
                const uint32_t run = jpeg_prog_run_of((bf & 4u) != 0u, b, b, n < kProgThreads ? c0 + n : next);
                runs[b] = (uint16_t)run;
                if (run) atomicAdd(&s_cnt[2u + k][jpeg_prog_eob_symbol(run)], 1u);
            }
            const uint32_t lowest = mask_first(s_busy);
            if (lowest < kProgThreads) next = c0 + lowest;
            __syncthreads();
            if (c0 == 0u) break;
        }
    }

    // ---- the DC counts (dc_code's difference and size) ----
    const int16_t *dcs = reinterpret_cast<const int16_t *>(rec + kJpegProgHeadWords);
    for (uint32_t u = tid; u < nunits; u += kProgThreads) {
        const int32_t diff = (int32_t)dcs[u] - (u >= 3u ? (int32_t)dcs[u - 3u] : 0);
        atomicAdd(&s_cnt[(u % 3u) ? 1u : 0u][coef_size(diff)], 1u);
    }
    __syncthreads();

    // ---- the six tables ----
    uint32_t rank[kJpegProgTables];
#pragma unroll
    for (uint32_t t = 0; t < kJpegProgTables; ++t) {
        uint32_t used;
        rank[t] = jpeg_opt_rank(s_cnt[t], tid, &used);
        if (s_cnt[t][tid]) s_A[t][1u + rank[t]] = s_cnt[t][tid];
        if (tid == 0u) { s_used[t] = used; s_A[t][0] = 1u; }
    }
    __syncthreads();
    if ((tid & 63u) == 0u)
        for (uint32_t t = wave; t < kJpegProgTables; t += kProgWaves) jpeg_opt_lengths(s_A[t], (int)s_used[t] + 1, s_code[t]);
    __syncthreads();
#pragma unroll
    for (uint32_t t = 0; t < kJpegProgTables; ++t) s_len[t][tid] = s_cnt[t][tid] ? (uint8_t)jpeg_opt_length_of_rank(s_code[t].num, rank[t]) : (uint8_t)0;
    __syncthreads();
#pragma unroll
    for (uint32_t t = 0; t < kJpegProgTables; ++t) {
        const uint32_t l = s_len[t][tid];
        uint32_t lut = 0u;
        if (l) {
            const uint32_t pos = jpeg_opt_pos(s_len[t], tid);
            lut = (l << 16) | (s_code[t].first_code[l] + pos);
            s_vals[t][s_code[t].first_idx[l] + pos] = (uint8_t)tid;
        }
        if (t < 2u) { if (tid < kDcCodes) rec[kJpegProgDcLut + kDcCodes * t + tid] = lut; }
        else rec[kJpegProgAcLut + 256u * (t - 2u) + tid] = lut;
    }
    __syncthreads();

    // ---- the five headers ----
    const uint8_t *hdr = reinterpret_cast<const uint8_t *>(arena + jb.tab_off);
    uint8_t *out = reinterpret_cast<uint8_t *>(rec + kJpegProgHeader);
    if (tid < kJpegOptPrefixBytes) out[tid] = tid == kJpegProgSofAt ? (uint8_t)0xC2 : hdr[tid];
    uint32_t at = kJpegOptPrefixBytes;
#pragma unroll
    for (uint32_t t = 0; t < kJpegProgTables; ++t) {
        const uint32_t used = s_used[t];
        if (t >= 2u) { out = reinterpret_cast<uint8_t *>(rec + kJpegProgHeader + kJpegProgDcHeaderWords + kJpegProgAcHeaderWords * (t - 2u)); at = 0u; }
        if (tid < kJpegOptDhtHead) out[at + tid] = jpeg_opt_dht_head(jpeg_prog_dht_slot(t), tid, s_code[t].num, used);
        if (tid < used) out[at + kJpegOptDhtHead + tid] = s_vals[t][tid];
        at += kJpegOptDhtHead + used;
        if (t == 0u) continue;                           // (DC chroma follows DC luma)
        if (t == 1u) { if (tid < kJpegProgDcSos) out[at + tid] = jpeg_prog_dc_sos(tid); at += kJpegProgDcSos; }
        else { if (tid < kJpegProgAcSos) out[at + tid] = jpeg_prog_ac_sos(t - 2u, tid); at += kJpegProgAcSos; }
        if (tid == 0u) rec[kJpegProgHdrLen + t - 1u] = at;
    }
}

// ---------------------------------------------------------------- kernel 3: coding --

// Codes AC scan k of one unit and the run its block carries into the scan's record of the block.
__device__ __forceinline__ void code_band(const JpegJob &jb, const uint32_t *s_ac, const int16_t *cf, uint64_t m, uint32_t k, uint32_t nblocks,
                                          uint32_t blk, const uint16_t *runs)
{
    const JpegProgBand band = jpeg_prog_band(k);
    const uint32_t *tab = s_ac + 256u * k;
    const size_t r = (size_t)k * nblocks + blk;
    UnitBits ub{0ull, 0u, 0u, 0u, (global_u32 *)jb.acbits + r * kAcWordsPerUnit, 0u, 0u, 0u};
    uint64_t bm = m & jpeg_prog_band_mask(band.ss, band.se);
    uint32_t prev = band.ss - 1u;
    while (bm) {
        const uint32_t pos = (uint32_t)__builtin_ctzll(bm);
        bm &= bm - 1ull;
        const int32_t cv = cf[pos];
        uint32_t run = pos - prev - 1u;
        prev = pos;
        if (run > 15u) {
            const uint32_t zrl = tab[0xF0];
            do { ub.put(zrl & 0xffffu, zrl >> 16); run -= 16u; } while (run > 15u);
        }
        const uint32_t mag = (uint32_t)(cv < 0 ? -cv : cv);
        const uint32_t size = 32u - (uint32_t)__clz(mag);
        const uint32_t value = (uint32_t)(cv + (cv >> 31)) & ((1u << size) - 1u);
        const uint32_t e = tab[(run << 4) | size];
        ub.put(((e & 0xffffu) << size) | value, (e >> 16) + size);          // <= 16 + 10 bits
    }
    const uint32_t run = runs[r];
    if (run) {
        const uint32_t n = 31u - (uint32_t)__clz(run);
        const uint32_t e = tab[n << 4];
        ub.put(((e & 0xffffu) << n) | (run - (1u << n)), (e >> 16) + n);    // <= 16 + 14 bits
    }
    if (ub.pend) ub.word((uint32_t)(ub.acc << (32u - ub.pend)));            // the last word, padded with zeros
    const u32x4 rec = {ub.total << 16, ub.w0, ub.w1, ub.w2};
    ((global_u32x4 *)jb.units)[r] = rec;
}

__global__ __launch_bounds__(kJpegThreads) void jpeg_prog_code_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                      uint32_t job_base, const uint32_t *__restrict__ prog)
{
    __shared__ WaveLds s_w[kWavesPerWg];
    __shared__ uint32_t s_ac[kJpegProgAcScans * 256u];   // the four AC scans' code tables
    const JpegJob jb = jobs[job_base + blockIdx.y];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t nblocks = jb.bx * jb.by;
    if (blockIdx.x * kBlocksPerWg >= nblocks) return;    // whole workgroup idle (uniform)
    const uint32_t *rec = prog + jb.opt_off;
    for (uint32_t i = threadIdx.x; i < kJpegProgAcScans * 256u; i += kJpegThreads) s_ac[i] = rec[kJpegProgAcLut + i];
    __syncthreads();
    const uint32_t first = blockIdx.x * kBlocksPerWg + wave * kBlocksPerWave;
    if (first >= nblocks) return;                        // wave-uniform; from here on waves never synchronise with each other
    const uint32_t count = min(kBlocksPerWave, nblocks - first);
    WaveLds &w = s_w[wave];
    if (jb.c == 4u && (reinterpret_cast<uintptr_t>(jb.src) & 3u) == 0u) transform_blocks<true>(jb, arena, first, count, lane, w);
    else transform_blocks<false>(jb, arena, first, count, lane, w);
    wave_lds_sync();
    const uint32_t b = lane & 15u, comp = lane >> 4;
    if (comp >= 3u || b >= count) return;
    const uint16_t *runs = reinterpret_cast<const uint16_t *>(rec + kJpegProgHeadWords) + (size_t)nblocks * 3u;
    const uint32_t u = b * 3u + comp;
    code_band(jb, s_ac, w.coef[u], w.nz[u], comp, nblocks, first + b, runs);
    if (comp == 0u) code_band(jb, s_ac, w.coef[u], w.nz[u], 3u, nblocks, first + b, runs);
}

// ---------------------------------------------------------------- kernel 4: offsets, assembly, stuffing, framing, scan after scan --

// Record u of scan `scan`: its code's bits; *dcw = a DC code, left-aligned (scan 0 only)
__device__ __forceinline__ uint32_t prog_record_bits(const JpegJob &jb, const uint32_t *s_dc, const int16_t *dcs, uint32_t scan, uint32_t nblocks, uint32_t u,
                                                     uint32_t *dcw)
{
    if (scan == 0u) {
        uint32_t len;
        *dcw = dc_code(s_dc, u, (uint32_t)(uint16_t)dcs[u], u >= 3u ? (uint32_t)(uint16_t)dcs[u - 3u] : 0u, &len);
        return len;
    }
    return ((const global_u32 *)(jb.units + ((size_t)(scan - 1u) * nblocks + u)))[0] >> 16;
}

__global__ __launch_bounds__(kPackThreads) void jpeg_prog_pack_kernel(const JpegJob *__restrict__ jobs, uint32_t job_base, const uint32_t *__restrict__ prog)
{
    __shared__ uint32_t s_win[kWinWords];
    __shared__ uint32_t s_w[kPackWaves], s_carry, s_lo, s_hi, s_dc[2u * kDcCodes];
    const JpegJob jb = jobs[job_base + blockIdx.x];
    const uint32_t tid = threadIdx.x, nblocks = jb.bx * jb.by, limit = jb.dst_cap;
    constexpr uint32_t T = kPackThreads;
    const uint32_t *rec = prog + jb.opt_off;
    const int16_t *dcs = reinterpret_cast<const int16_t *>(rec + kJpegProgHeadWords);
    if (tid < 2u * kDcCodes) s_dc[tid] = rec[kJpegProgDcLut + tid];
    uint64_t out_at = 0;                                  // (uniform) bytes of the file so far
    for (uint32_t scan = 0; scan < kJpegProgScans; ++scan) {
        const uint32_t nrec = scan == 0u ? nblocks * 3u : nblocks;
        // ---- the scan's header ----
        const uint8_t *hdr = reinterpret_cast<const uint8_t *>(rec + kJpegProgHeader + (scan ? kJpegProgDcHeaderWords + kJpegProgAcHeaderWords * (scan - 1u) : 0u));
        const uint32_t hdr_bytes = rec[kJpegProgHdrLen + scan];
        for (uint32_t i = tid; i < hdr_bytes; i += T) if (out_at + i < limit) jb.dst[out_at + i] = hdr[i];
        out_at += hdr_bytes;
        // ---- bit offset of every record: exclusive scan of the code sizes ----
        if (tid == 0u) s_carry = 0u;
        __syncthreads();
        for (uint32_t base = 0; base < nrec; base += T) {
            const uint32_t u = base + tid;
            uint32_t dcw;
            const uint32_t len = u < nrec ? prog_record_bits(jb, s_dc, dcs, scan, nblocks, u, &dcw) : 0u;
            uint32_t chunk;
            const uint32_t ex = wg_exclusive_scan(len, s_w, &chunk);
            const uint32_t carry = s_carry;
            if (u < nrec) ((global_u32 *)jb.unit_off)[u] = carry + ex;
            __syncthreads();
            if (tid == 0u) s_carry = carry + chunk;
            __syncthreads();
        }
        const uint32_t total_bits = s_carry;
        if (tid == 0u) jb.unit_off[nrec] = total_bits;
        __threadfence_block();
        __syncthreads();
        const uint32_t nbytes = (total_bits + 7u) >> 3;
        uint32_t ff_before = 0; // stuffed bytes emitted by earlier windows (same value in every thread)
        for (uint32_t wbase = 0; wbase * 32ull < total_bits; wbase += kWinWords) {
            const uint64_t wb = (uint64_t)wbase * 32u, we = wb + (uint64_t)kWinWords * 32u;
            for (uint32_t i = tid; i < kWinWords; i += T) s_win[i] = 0u;
            // records that touch this window: offsets are ascending, so two binary searches bound them
            if (tid == 0u) {
                uint32_t lo = 0, hi = nrec;              // first u with unit_off[u + 1] > wb
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (jb.unit_off[mid + 1u] > wb) hi = mid; else lo = mid + 1u; }
                s_lo = lo;
                uint32_t lo2 = lo, hi2 = nrec;           // first u with unit_off[u] >= we
                while (lo2 < hi2) { const uint32_t mid = (lo2 + hi2) >> 1; if (jb.unit_off[mid] >= we) hi2 = mid; else lo2 = mid + 1u; }
                s_hi = lo2;
            }
            __syncthreads();
            const uint32_t u_lo = s_lo, u_hi = s_hi;
            for (uint32_t u = u_lo + tid; u < u_hi; u += T) {
                const uint32_t off = jb.unit_off[u];
                if (scan == 0u) {
                    uint32_t dcw;
                    prog_record_bits(jb, s_dc, dcs, 0u, nblocks, u, &dcw);
                    win_or(s_win, wbase, off, dcw);
                } else {
                    const size_t r = (size_t)(scan - 1u) * nblocks + u;
                    const u32x4 p = ((const global_u32x4 *)jb.units)[r];
                    const uint32_t nw = ((p.x >> 16) + 31u) >> 5;
                    // (a record's unused words are zero and win_or places no zero word)
                    win_or(s_win, wbase, off, p.y);
                    win_or(s_win, wbase, (uint64_t)off + 32u, p.z);
                    win_or(s_win, wbase, (uint64_t)off + 64u, p.w);
                    for (uint32_t w = kUnitAcWords; w < nw; ++w)
                        win_or(s_win, wbase, (uint64_t)off + 32u * w, ((const global_u32 *)jb.acbits)[r * kAcWordsPerUnit + w]);
                }
            }
            __syncthreads();
            // BitWriter::pad_byte: the scan's last partial byte is filled with ones
            if (tid == 0u && (total_bits & 7u) && (total_bits >> 5) >= wbase && (total_bits >> 5) < wbase + kWinWords)
                s_win[(total_bits >> 5) - wbase] |= (0xFFu >> (total_bits & 7u)) << (24u - 8u * ((total_bits >> 3) & 3u));
            __syncthreads();
            // 0xFF -> 0xFF 0x00 stuffing: scan of the 0xFF counts, then every thread writes its four bytes
            const uint32_t win_bytes = (uint32_t)min((uint64_t)kWinWords * 4u, (uint64_t)nbytes - (uint64_t)wbase * 4u);
            if (tid == 0u) s_carry = 0u;
            __syncthreads();
            for (uint32_t base = 0; base < win_bytes; base += 4u * T) {
                const uint32_t i = base + tid * 4u;
                const uint32_t word = i < win_bytes ? s_win[i >> 2] : 0u;     // stream order = most significant byte first
                const uint32_t valid = i < win_bytes ? (win_bytes - i < 4u ? win_bytes - i : 4u) : 0u;
                uint32_t ff = 0;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) ff += (k < valid && ((word >> (24u - 8u * k)) & 255u) == 255u) ? 1u : 0u;
                uint32_t chunk;
                const uint32_t ex = wg_exclusive_scan(ff, s_w, &chunk);
                const uint32_t carry = s_carry;
                uint64_t o = out_at + (uint64_t)wbase * 4u + i + ff_before + carry + ex;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    if (k < valid) {
                        const uint32_t b = (word >> (24u - 8u * k)) & 255u;
                        if (o < limit) jb.dst[o] = (uint8_t)b;
                        ++o;
                        if (b == 255u) { if (o < limit) jb.dst[o] = 0u; ++o; }
                    }
                }
                __syncthreads();
                if (tid == 0u) s_carry = carry + chunk;
                __syncthreads();
            }
            ff_before += s_carry;
            __syncthreads();
        }
        out_at += (uint64_t)nbytes + ff_before;
    }
    if (tid == 0u) {
        if (out_at + 2u <= limit) {
            jb.dst[out_at] = 0xFF; jb.dst[out_at + 1u] = 0xD9; // EOI
            jb.result[1] = (uint32_t)(out_at + 2u);
        } else {
            jb.result[1] = 0u;
            atomicOr(&jb.result[0], FL_JPEG_RESULT_OVERFLOW);
        }
    }
}

} // namespace

hipError_t launch_jpeg_encode_progressive(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_blocks,
                                          uint32_t *prog, uint32_t *hist, hipStream_t st)
{
    if (!njobs || !max_blocks) return hipSuccess;
    const dim3 grid((max_blocks + kBlocksPerWg - 1) / kBlocksPerWg, njobs);
    if (hipError_t e = hipMemsetAsync(hist, 0, (size_t)njobs * kJpegProgHistWords * sizeof(uint32_t), st)) return e;
    hipLaunchKernelGGL(jpeg_prog_stats_kernel, grid, dim3(kJpegThreads), 0, st, jobs, arena, job_base, prog, hist);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_prog_tables_kernel, dim3(njobs), dim3(kProgThreads), 0, st, jobs, arena, job_base, prog, (const uint32_t *)hist);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_prog_code_kernel, grid, dim3(kJpegThreads), 0, st, jobs, arena, job_base, (const uint32_t *)prog);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_prog_pack_kernel, dim3(njobs), dim3(kPackThreads), 0, st, jobs, job_base, (const uint32_t *)prog);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace fl
