// fl_jpeg_prog_core.h -- progressive files of the JPEG encoder (FLGPU_FEO_JPEG_PROGRESSIVE on FLGPU_FE_JPEG): the scan script, the band
// and end-of-band run rules of T.81 G.1.2.2 and the segment bytes, as code that compiles for the host and for the device.
// fl_jpeg_prog.hip runs it over the pictures of a batch; jpeg_prog_encode_serial below restates the whole coder in plain loops for
// flgpu_debug_jpeg_progressive_scans (fl_encode.cpp) and tests/jpeg_prog_host.cpp; tests/jpeg_prog_model.py restates it in numpy.
//
// The file: the baseline header's 177 prefix bytes with SOF0's marker turned into SOF2's, then five scans by spectral selection
// (Ah = Al = 0), each behind its own DHT segment(s) and SOS:
//   scan 0: DC of Y, Cb, Cr interleaved (tables: DC destination 0 from the Y differences, destination 1 from Cb + Cr), coded as the
//           baseline codes DC terms;
//   scans 1-4: Y 1-5, Cb 1-63, Cr 1-63, Y 6-63, one component each, blocks in raster order, AC destination 0 redefined every time.
// An AC scan (libjpeg's encode_mcu_AC_first without restarts): a block's non-zero coefficients of the band as the baseline codes
// them (ZRL only in front of a coefficient); a block whose band ends in a zero -- an empty band included -- lengthens the pending
// end-of-band run by one; the run goes out in front of the next block that holds a coefficient in the band, when it reaches 32,767
// and at the scan's end, as symbol n << 4 (n = floor(log2 run)) and n bits of run - 2^n.
// Per block instead of in sequence (jpeg_prog_run_of): the blocks between a run's first block and the block that ends it emit
// nothing, so the run's code sits directly behind its first block's coefficient codes -- and every 32,767th block of a long run
// carries the next part's code.  So a block carries at most one run code per scan.
// Every table is fl_jpeg_opt_core.h's rule from the scan's own counts.  Each scan ends as the baseline's does (ones to the byte
// edge, 0xFF -> 0xFF00); EOI closes the file.
#pragma once
#include <stdint.h>

#include "fl_jpeg_opt_core.h"

namespace fl {

constexpr uint32_t kJpegProgScans = 5, kJpegProgAcScans = 4, kJpegProgTables = 6; // tables: 0 DC luma, 1 DC chroma, 2 .. 5 the AC scans'
constexpr uint32_t kJpegProgEobLimit = 32767;    // blocks per end-of-band run: EOB14 with all fourteen extra bits set
constexpr uint32_t kJpegProgSofAt = 21;          // the prefix byte that says SOF0 (0xC0) / SOF2 (0xC2)
constexpr uint32_t kJpegProgDcSos = 14, kJpegProgAcSos = 10;
// An AC table's symbols: 16 runs x 10 sizes (|AC| <= 1023 for 8-bit samples), ZRL, EOB0 .. EOB14; a DC table's: sizes 0 .. 11
constexpr uint32_t kJpegProgAcSymbols = 176, kJpegProgDcSymbols = 12;
constexpr uint32_t kJpegProgDcHeaderMax = kJpegOptPrefixBytes + 2u * (kJpegOptDhtHead + kJpegProgDcSymbols) + kJpegProgDcSos;   // 257
constexpr uint32_t kJpegProgAcHeaderMax = kJpegOptDhtHead + kJpegProgAcSymbols + kJpegProgAcSos;                                // 207
constexpr uint32_t kJpegProgHeaderMax = kJpegProgDcHeaderMax + kJpegProgAcScans * kJpegProgAcHeaderMax;                         // 1,085
// flgpu_plan::max_out_bytes.  A unit's longest code, all scans together: a DC code of 16 + 11 bits (the picture's own table may give
// the size symbol 16 bits where Annex K's longest is 11), 63 coefficients of 16 + 10 bits, and one run code of 16 + 14 bits per AC scan
// the unit is in -- two for Y: 27 + 1,638 + 60 = 1,725 bits.  Every scan is padded to a byte (at most one byte each) and every byte
// may be stuffed; the headers and EOI are not.
constexpr uint32_t kJpegProgMaxUnitBytes = 216;
static_assert(16u + 11u + 63u * 26u + 2u * (16u + 14u) <= kJpegProgMaxUnitBytes * 8u, "a unit's longest code");
constexpr uint32_t kJpegProgFixedBytes = 1104;   // >= the headers, EOI and the five scans' padding bytes, stuffed
static_assert(kJpegProgHeaderMax + 2u + 2u * kJpegProgScans <= kJpegProgFixedBytes, "what a file holds besides its units' codes");

struct JpegProgBand { uint32_t comp, ss, se; };
// AC scan k (0 .. 3; the file's scan k + 1)
FL_JOPT_HD JpegProgBand jpeg_prog_band(uint32_t k)
{
    return k == 0u ? JpegProgBand{0u, 1u, 5u} : k == 3u ? JpegProgBand{0u, 6u, 63u} : JpegProgBand{k, 1u, 63u};
}
FL_JOPT_HD uint64_t jpeg_prog_band_mask(uint32_t ss, uint32_t se) { return (se == 63u ? ~0ull : (1ull << (se + 1u)) - 1ull) & ~((1ull << ss) - 1ull); }

// What the run rule needs of (scan, block), from the block's mask of non-zero coefficients
constexpr uint32_t kJpegProgEmpty = 1u, kJpegProgTail = 2u;    // no coefficient in the band; the band's last coefficient is zero
FL_JOPT_HD uint32_t jpeg_prog_flags(uint64_t nz, uint32_t ss, uint32_t se)
{
    return ((nz & jpeg_prog_band_mask(ss, se)) ? 0u : kJpegProgEmpty) | (((nz >> se) & 1ull) ? 0u : kJpegProgTail);
}

// The first block of the run an empty block lies in: prev = the last block in front of it that holds a coefficient in the band
// (-1: none), prev_tail = whether that block's band ends in a zero
FL_JOPT_HD uint32_t jpeg_prog_run_head(int64_t prev, bool prev_tail) { return (uint32_t)(prev >= 0 && prev_tail ? prev : prev + 1); }
// The length of the run whose code block b carries behind its coefficient codes (0: none).  tail: b's band ends in a zero; head: the
// first block of the run b lies in (b itself if it holds a coefficient); next: the first block behind b that holds a coefficient in
// the band (the number of blocks: none).
FL_JOPT_HD uint32_t jpeg_prog_run_of(bool tail, uint32_t b, uint32_t head, uint32_t next)
{
    if (!tail || (b - head) % kJpegProgEobLimit != 0u) return 0u;
    const uint32_t left = next - b;
    return left < kJpegProgEobLimit ? left : kJpegProgEobLimit;
}
FL_JOPT_HD uint32_t jpeg_prog_log2(uint32_t run) { uint32_t n = 0; while (run >> (n + 1u)) ++n; return n; } // run >= 1
FL_JOPT_HD uint32_t jpeg_prog_eob_symbol(uint32_t run) { return jpeg_prog_log2(run) << 4; }

// Segment bytes.  Byte i of the SOS of scan 0 / of AC scan k
FL_JOPT_HD uint8_t jpeg_prog_dc_sos(uint32_t i)
{
    const uint8_t s[kJpegProgDcSos] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x10, 3, 0x10, 0, 0, 0};
    return s[i];
}
FL_JOPT_HD uint8_t jpeg_prog_ac_sos(uint32_t k, uint32_t i)
{
    const JpegProgBand b = jpeg_prog_band(k);
    const uint8_t s[kJpegProgAcSos] = {0xFF, 0xDA, 0, 8, 1, (uint8_t)(b.comp + 1u), 0x00, (uint8_t)b.ss, (uint8_t)b.se, 0};
    return s[i];
}
// fl_jpeg_opt_core.h numbers tables in the baseline's DHT order (class = t & 1, destination = t >> 1): what table t here is there
FL_JOPT_HD uint32_t jpeg_prog_dht_slot(uint32_t t) { return t == 0u ? 0u : t == 1u ? 2u : 1u; }

// ---- the host twin -------------------------------------------------------------------------------------------------------------

// One table through the rule: cnt[256] -> lut[256] (length << 16 | code), its DHT segment (at most 21 + 256 bytes); returns the
// segment's bytes, 0 if the counts sum to 2^32 - 1 or more
inline uint32_t jpeg_prog_table_serial(const uint32_t *cnt, uint32_t slot, uint32_t *lut, uint8_t *dht)
{
    uint32_t A[kJpegOptMaxLeaves + 1u], rank[256], used = 0;
    uint8_t len[256];
    JpegOptCode code;
    uint64_t sum = 0;
    for (uint32_t s = 0; s < 256u; ++s) sum += cnt[s];
    if (sum >= 0xffffffffull) return 0;
    A[0] = 1u;
    for (uint32_t s = 0; s < 256u; ++s) {
        rank[s] = jpeg_opt_rank(cnt, s, &used);
        if (cnt[s]) A[1u + rank[s]] = cnt[s];
    }
    jpeg_opt_lengths(A, (int)used + 1, code);
    for (uint32_t s = 0; s < 256u; ++s) len[s] = cnt[s] ? (uint8_t)jpeg_opt_length_of_rank(code.num, rank[s]) : (uint8_t)0;
    for (uint32_t i = 0; i < kJpegOptDhtHead; ++i) dht[i] = jpeg_opt_dht_head(slot, i, code.num, used);
    for (uint32_t s = 0; s < 256u; ++s) {
        lut[s] = 0u;
        if (!len[s]) continue;
        const uint32_t pos = jpeg_opt_pos(len, s);
        lut[s] = ((uint32_t)len[s] << 16) | (code.first_code[len[s]] + pos);
        dht[kJpegOptDhtHead + code.first_idx[len[s]] + pos] = (uint8_t)s;
    }
    return kJpegOptDhtHead + used;
}

// BitWriter of the baseline coder: most significant bit first, ones to the byte edge, 0xFF -> 0xFF00.  out holds cap bytes; n counts on.
struct JpegProgWriter {
    uint8_t *out; uint64_t cap, n;
    uint64_t acc; uint32_t pend;
    void byte(uint8_t b) { if (n < cap) out[n] = b; ++n; }
    void put(uint32_t code, uint32_t len)
    {
        acc = (acc << len) | code; pend += len;
        while (pend >= 8u) { pend -= 8u; const uint8_t b = (uint8_t)(acc >> pend); byte(b); if (b == 0xFFu) byte(0); }
    }
    void pad() { if (pend) put(0x7Fu >> (pend - 1u), 8u - pend); }
};

// One (table, symbol, value, value bits) step of a scan: counted in the first pass, coded in the second
struct JpegProgSink {
    uint32_t *cnt;             // pass 1: cnt[table][256]
    const uint32_t *lut;       // pass 2: lut[table][256]
    JpegProgWriter *w;
    void symbol(uint32_t t, uint32_t s, uint32_t value, uint32_t vbits)
    {
        if (cnt) { cnt[256u * t + s]++; return; }
        const uint32_t e = lut[256u * t + s];
        w->put(e & 0xffffu, e >> 16);
        if (vbits) w->put(value, vbits);
    }
};

inline uint32_t jpeg_prog_size(int32_t v) { uint32_t m = (uint32_t)(v < 0 ? -v : v), n = 0; while (m) { ++n; m >>= 1; } return n; }
inline uint32_t jpeg_prog_value(int32_t v, uint32_t size) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u); }

// Scan `scan` (0: DC; 1 .. 4: AC scan - 1) of coef[3 * nblocks][64] (unit = 3 * block + component, zig-zag), block by block as the
// device does it: flags, then each block's run from the blocks around it, then its symbols -- table index 0 / 1 (DC) or scan + 1.
inline void jpeg_prog_scan_serial(const int16_t *coef, uint32_t nblocks, uint32_t scan, JpegProgSink &sink)
{
    if (scan == 0u) {
        int32_t prev[3] = {0, 0, 0};
        for (uint32_t u = 0; u < 3u * nblocks; ++u) {
            const int32_t dc = coef[(size_t)u * 64u], diff = dc - prev[u % 3u];
            prev[u % 3u] = dc;
            const uint32_t size = jpeg_prog_size(diff);
            sink.symbol(u % 3u ? 1u : 0u, size, jpeg_prog_value(diff, size), size);
        }
        return;
    }
    const JpegProgBand band = jpeg_prog_band(scan - 1u);
    auto mask_of = [&](uint32_t b) {
        const int16_t *c = coef + ((size_t)b * 3u + band.comp) * 64u;
        uint64_t m = 0;
        for (uint32_t k = 1; k < 64u; ++k) if (c[k]) m |= 1ull << k;
        return m;
    };
    int64_t prev = -1;          // the last block so far that holds a coefficient in the band
    bool prev_tail = false;
    uint32_t next = 0;          // the first such block at or behind b + 1
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint64_t nz = mask_of(b);
        const uint32_t bf = jpeg_prog_flags(nz, band.ss, band.se);
        if (next <= b) { next = b + 1u; while (next < nblocks && (jpeg_prog_flags(mask_of(next), band.ss, band.se) & kJpegProgEmpty)) ++next; }
        const bool empty = (bf & kJpegProgEmpty) != 0u, tail = (bf & kJpegProgTail) != 0u;
        const uint32_t head = empty ? jpeg_prog_run_head(prev, prev_tail) : b;
        const uint32_t run = jpeg_prog_run_of(tail, b, head, next);
        const int16_t *c = coef + ((size_t)b * 3u + band.comp) * 64u;
        uint32_t zeros = 0;
        for (uint32_t k = band.ss; k <= band.se; ++k) {
            if (!c[k]) { ++zeros; continue; }
            while (zeros > 15u) { sink.symbol(scan + 1u, 0xF0u, 0u, 0u); zeros -= 16u; }
            const uint32_t size = jpeg_prog_size(c[k]);
            sink.symbol(scan + 1u, (zeros << 4) | size, jpeg_prog_value(c[k], size), size);
            zeros = 0;
        }
        if (run) { const uint32_t n = jpeg_prog_log2(run); sink.symbol(scan + 1u, n << 4, run - (1u << n), n); }
        if (!empty) { prev = b; prev_tail = tail; }
    }
}

// The whole file in plain loops.  prefix: the baseline header's first 177 bytes.  Out: counts[6][256], the file (cap bytes at out;
// *bytes = its length, which may exceed cap: then nothing beyond cap was written).  -1: a table's counts sum to 2^32 - 1 or more.
inline int jpeg_prog_encode_serial(const int16_t *coef, uint32_t nblocks, const uint8_t *prefix, uint32_t *counts, uint8_t *out, uint64_t cap,
                                   uint64_t *bytes)
{
    for (uint32_t i = 0; i < kJpegProgTables * 256u; ++i) counts[i] = 0u;
    JpegProgSink count{counts, nullptr, nullptr};
    for (uint32_t scan = 0; scan < kJpegProgScans; ++scan) jpeg_prog_scan_serial(coef, nblocks, scan, count);
    JpegProgWriter w{out, cap, 0, 0, 0};
    for (uint32_t i = 0; i < kJpegOptPrefixBytes; ++i) w.byte(i == kJpegProgSofAt ? 0xC2u : prefix[i]);
    uint32_t luts[kJpegProgTables * 256u];
    for (uint32_t t = 0; t < kJpegProgTables; ++t) {
        uint8_t dht[kJpegOptDhtHead + 256u];
        const uint32_t n = jpeg_prog_table_serial(counts + 256u * t, jpeg_prog_dht_slot(t), luts + 256u * t, dht);
        if (!n) return -1;
        for (uint32_t i = 0; i < n; ++i) w.byte(dht[i]);
        if (t == 0u) continue;                         // DC chroma follows DC luma
        const uint32_t scan = t - 1u;
        if (scan == 0u) for (uint32_t i = 0; i < kJpegProgDcSos; ++i) w.byte(jpeg_prog_dc_sos(i));
        else for (uint32_t i = 0; i < kJpegProgAcSos; ++i) w.byte(jpeg_prog_ac_sos(scan - 1u, i));
        JpegProgSink code{nullptr, luts, &w};
        jpeg_prog_scan_serial(coef, nblocks, scan, code);
        w.pad();
    }
    w.byte(0xFF); w.byte(0xD9);
    *bytes = w.n;
    return 0;
}

} // namespace fl
