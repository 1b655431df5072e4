// fl_jpeg.h -- launch interface between the host runtime and the JPEG encoder on the device (fl_jpeg.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fl {

// One image of a JPEG-encode launch (fl_jpeg.hip).
#define FL_JPEG_RESULT_OVERFLOW 4u
#define FL_JPEG_RESULT_OPTIMIZED 8u   // FLGPU_FEO_JPEG_OPTIMIZE: the file went out with the picture's own Huffman tables
constexpr uint32_t kAcWordsPerUnit = 52; // 63 coefficients x (16-bit code + 10 value bits) = 1638 bits
constexpr uint32_t kUnitAcWords = 3;     // AC code words a unit's record holds itself (96 bits: nearly every unit of a photograph)
// What jpeg_dct_quant_kernel hands jpeg_pack_kernel per unit (unit = block * 3 + component): one 16-byte record, written and
// read with one access.  A unit whose AC code is longer than 96 bits continues in its JpegJob::acbits slot, from word 3 on.
struct alignas(16) JpegUnit {
    uint32_t meta;                // quantised DC (low 16 bits, i16) | AC code bits << 16
    uint32_t ac[kUnitAcWords];    // the AC code's first 96 bits from bit 0, most significant bit first; unused bits are zero
};
struct alignas(16) JpegJob {
    const uint8_t *src;   // interleaved pixels, w x h x c
    uint8_t *dst;         // the JFIF stream
    JpegUnit *units;      // scratch: [unit] the unit's record; unit = block * 3 + component (FLGPU_FEO_JPEG_420: MCU * 6 + slot)
    uint32_t *unit_off;   // scratch: units + 1 bit offsets
    uint32_t *acbits;     // scratch: [unit][kAcWordsPerUnit] the unit's AC code from bit 0, most significant bit first; only words
                          // kUnitAcWords and up are written and read here (the slot keeps its worst-case size and every index)
    uint32_t *result;     // [0] |= flags (FL_JPEG_RESULT_OVERFLOW), [1] = stream bytes (0 if it did not fit dst_cap)
    uint32_t w, h, c;
    uint32_t bx, by;      // blocks per row / column (FLGPU_FEO_JPEG_420: MCUs of 16 x 16)
    uint32_t tab_off;     // arena word offset of the header + quantisation tables block (fl_jpeg_tables.h)
    uint32_t opt_off;     // FLGPU_FEO_JPEG_OPTIMIZE only (else 0): word offset of the picture's record in the batch's optimise scratch
                          // (FLGPU_FEO_JPEG_PROGRESSIVE: in the batch's progressive scratch)
    uint32_t dst_cap;     // bytes available at dst
};

// FLGPU_FEO_JPEG_OPTIMIZE.  A picture's record in the optimise scratch, in words from JpegJob::opt_off: what jpeg_opt_tables_kernel
// leaves for the coding and pack launches -- header length and decision, the two DC and the two AC code tables (length << 16 | code),
// the header bytes (prefix, four DHT segments, SOS; Annex K's where the decision fell against the picture's tables) -- and behind them
// the quantised DC terms, 2 bytes per unit, which jpeg_opt_stats_kernel leaves for the DC histograms.
constexpr uint32_t kJpegOptHdrLen = 0, kJpegOptFlag = 1, kJpegOptDcLut = 4, kJpegOptAcLut = 32, kJpegOptHeader = 544, kJpegOptHeadWords = 704;
constexpr uint32_t kJpegOptHistWords = 512; // per picture, in a scratch of its own (cleared per batch): the AC symbol counts, luma then chroma
constexpr size_t jpeg_opt_bytes(size_t units) { return (kJpegOptHeadWords * 4u + units * 2u + 255u) & ~(size_t)255u; }

// JPEG encode of njobs pictures: colour + FDCT + quantise + AC coding (one wave per 16 blocks), then offsets, assembly, stuffing
// and framing (one workgroup per picture)
hipError_t launch_jpeg_encode(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_blocks,
                              hipStream_t st);
// The same for pictures that carry FLGPU_FEO_JPEG_OPTIMIZE (jobs job_base .. job_base + njobs - 1, whose opt_off address `opt`; hist:
// njobs x kJpegOptHistWords words): clear the counts, count the AC symbols (the transform phase again, LDS histograms), build the four
// tables per picture and decide (one workgroup per picture), code with those tables, pack with the picture's header.
// fallback: the decision always falls against the picture's tables (tests).
hipError_t launch_jpeg_encode_optimized(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_blocks,
                                        uint32_t *opt, uint32_t *hist, bool fallback, hipStream_t st);

// FLGPU_FEO_JPEG_420 (fl_jpeg_420.hip): the same two sequences for pictures coded 4:2:0.  Their jobs' bx, by count 16 x 16 MCUs, a
// picture has 6 units per MCU (Y Y Y Y Cb Cr) in units, unit_off, acbits and its optimise record, and tab_off names a header whose SOF0
// says 2 x 2 for the first component.  max_mcus: the largest bx * by of the jobs.
hipError_t launch_jpeg_encode_420(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_mcus, hipStream_t st);
hipError_t launch_jpeg_encode_420_optimized(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_mcus,
                                            uint32_t *opt, uint32_t *hist, bool fallback, hipStream_t st);

// FLGPU_FEO_JPEG_PROGRESSIVE (fl_jpeg_prog.hip, fl_jpeg_prog_core.h): a progressive file of five scans.  A picture's jobs' units,
// unit_off and acbits hold four records per block, record = AC scan * blocks + block (the DC scan reads the DC terms), and opt_off names
// its record in the progressive scratch, in words: the five scans' header lengths, the two DC and the four AC code tables
// (length << 16 | code), the scans' header bytes (scan 0: prefix with SOF2, two DHT, SOS; scans 1-4: DHT, SOS), and behind them the
// quantised DC terms (2 bytes per unit) and one 16-bit word per (AC scan, block): the band's flags from the statistics launch, then
// the length of the end-of-band run the block codes (0: none).
constexpr uint32_t kJpegProgHdrLen = 0, kJpegProgDcLut = 8, kJpegProgAcLut = 32, kJpegProgHeader = 1056, kJpegProgDcHeaderWords = 80,
                   kJpegProgAcHeaderWords = 72, kJpegProgHeadWords = 1424;
static_assert(kJpegProgHeader + kJpegProgDcHeaderWords + 4u * kJpegProgAcHeaderWords == kJpegProgHeadWords, "the record's head");
constexpr uint32_t kJpegProgHistWords = 1024; // per picture, in a scratch of its own (cleared per batch): the four AC scans' symbol counts
constexpr size_t jpeg_prog_bytes(size_t blocks) { return (kJpegProgHeadWords * 4u + blocks * (3u * 2u + 4u * 2u) + 255u) & ~(size_t)255u; }
// max_blocks: the largest bx * by of the jobs; hist: njobs x kJpegProgHistWords words.  Launches: clear the counts, statistics (the
// transform phase, band symbols counted in LDS, DC terms and band flags), tables (one workgroup per picture: the runs, six tables,
// five headers), coding (the transform again, one record per AC scan and block), packing (one workgroup per picture, scan after scan).
hipError_t launch_jpeg_encode_progressive(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_blocks,
                                          uint32_t *prog, uint32_t *hist, hipStream_t st);

} // namespace fl
