// fl_pngsrc.h -- host half of the PNG decode front end (reference src/handler.rs:218-220: image 0.25.6 -> png 0.17 with
// Transformations::EXPAND): container parsing, chunk CRCs, and our own inflate.  The serial entropy stage runs here, on the
// calling thread; what it leaves -- the FILTERED scanlines behind a small header -- is what crosses PCIe, and the device
// (fl_pngdec.hip) undoes the row filters and expands palette / sub-byte / tRNS pictures to pixels.
// No HIP in this file or in fl_pngsrc.cpp: both compile alone with a plain C++ compiler (tests/png_host_fuzz.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fl_png_adam7.h"

namespace fl {

struct PngInfo {
    uint32_t width = 0, height = 0;
    uint32_t color_type = 0, bit_depth = 0;
    uint32_t channels = 0;     // of the picture the pipeline sees (1 Luma8, 2 LumaA8, 3 Rgb8, 4 Rgba8); 0 if unsupported
    uint32_t interlaced = 0;   // Adam7
    uint32_t has_trns = 0;
    uint32_t supported = 0;    // 1 = FLGPU_IMG_PNG_SOURCE decodes it: depth <= 8, no interlace (or, asked with adam7 = true, Adam7)
    uint32_t row_bytes = 0;    // ceil(width * samples * depth / 8): a scanline without its filter byte
    uint32_t bpp = 0;          // the filters' pixel distance in bytes: max(1, samples * depth / 8)
    uint32_t plte_entries = 0;
    uint32_t pixel_bits = 0;   // samples * depth
    uint64_t idat_bytes = 0;   // summed IDAT payloads
};

// Return codes of the host half: 0 = ok, kPngParse = not a PNG / damaged (FLGPU_ERR_PARSE), kPngUnsupported = well-formed
// but not covered (FLGPU_ERR_UNSUPPORTED), kPngSmall = the caller's buffer is too small.
constexpr int kPngParse = -1, kPngUnsupported = -2, kPngSmall = -3;

constexpr uint32_t kPngMagic = 0x31444e50u; // "PND1"
// A source that carries FLGPU_IMG_PNG_INFLATE is staged compressed: the same header under this magic, then the IDAT payloads back to back
// (total_bytes - header - kPngzPad bytes of them), then kPngzPad zero bytes so the kernel may read whole words past the end.
constexpr uint32_t kPngzMagic = 0x5a444e50u; // "PNDZ"
constexpr uint32_t kPngzPad = 16;
// the decoded picture may not exceed what the reference's decoder runs under (image::Limits::default(): 512 MiB), and the
// pipeline addresses pictures below 2^31 bytes
constexpr uint64_t kPngMaxDecoded = 1ull << 31;

// What crosses PCIe in front of the scanlines.  The palette is always full: tRNS folded into its alpha, entries PLTE does
// not have are opaque black, so a lookup with any 8-bit index stays inside the table.
struct alignas(16) PngBlobHeader {
    uint32_t magic;
    uint32_t width, height;
    uint32_t color_type, bit_depth;
    uint32_t channels;        // output channels
    uint32_t bpp, row_bytes;
    uint32_t has_trns;
    uint32_t key[3];          // tRNS of colour types 0 (key[0]) and 2: the raw sample values, compared before scaling
    uint32_t direct;          // 1 = the unfiltered rows ARE the pixels (8-bit colour type 0 / 2 / 4 / 6 without tRNS)
    uint32_t scan_off;        // byte offset of the scanlines: height x (1 + row_bytes), or the seven passes' (adam7_pass of width, height, depth)
    uint32_t total_bytes;     // header + scanlines
    uint32_t interlaced;      // 1 = Adam7: the scanlines are those of the passes, back to back (fl_png_adam7.h)
    uint32_t palette[256];    // r | g << 8 | b << 16 | a << 24
};

// Header inspection: signature, IHDR, and a walk over the chunks up to IEND (lengths and the CRCs of the chunks that are
// interpreted: IHDR, PLTE, tRNS, IDAT, IEND).
// verify_crc = false: layout and lengths only, for a caller that sizes its buffers from the header and then calls
// png_decode_scanlines, which verifies every CRC itself: the file is summed once per request.
// adam7 = true: an Adam7-interlaced file of depth <= 8 is supported too, its size bounds taken on the seven passes' scanlines.
int png_parse_info(const uint8_t *data, size_t n, PngInfo &info, bool verify_crc = true, bool adam7 = false);

// Bits per pixel of the blob's samples as stored (pixel_bits of PngInfo)
FL_A7_HD uint32_t png_pixel_bits(const PngBlobHeader &h) { return h.bit_depth < 8u ? h.bit_depth : 8u * h.bpp; }

// Bytes of the scanlines / of the whole blob for `info`.
inline size_t png_scan_bytes(const PngInfo &info)
{
    if (info.interlaced) return (size_t)adam7_scan_bytes(info.width, info.height, info.pixel_bits);
    return (size_t)info.height * (1u + (size_t)info.row_bytes);
}
inline size_t png_blob_bytes(const PngInfo &info) { return sizeof(PngBlobHeader) + png_scan_bytes(info); }

// Inflates the IDAT stream of a supported file into scan[0 .. png_scan_bytes) and checks Adler-32 and the filter bytes;
// hdr (optional) receives the header of the blob.  `scan` is the inflate window: nothing else is allocated.
// adam7 = true: as for png_parse_info; the stream of an interlaced file is left as it is stored, pass after pass.
int png_decode_scanlines(const uint8_t *data, size_t n, uint8_t *scan, size_t cap, PngBlobHeader *hdr, bool adam7 = false);

// Bytes of the staging of a source whose deflate stream the device inflates (fl_inflate.h): header + IDAT payloads + pad.
inline size_t png_stage_bytes(const PngInfo &info) { return sizeof(PngBlobHeader) + (size_t)info.idat_bytes + kPngzPad; }
// The host half of such a source: the same container walk with the same CRC checks as png_decode_scanlines, then the IDAT payloads
// copied back to back behind the header (magic kPngzMagic).  Nothing is inflated here.  blob[0 .. png_stage_bytes) is written.
int png_stage_compressed(const uint8_t *data, size_t n, uint8_t *blob, size_t cap, PngBlobHeader *hdr, bool adam7 = false);
// Bytes of the scanlines a blob header stands for.
inline size_t png_header_scan_bytes(const PngBlobHeader &h)
{
    if (h.interlaced) return (size_t)adam7_scan_bytes(h.width, h.height, png_pixel_bits(h));
    return (size_t)h.height * (1u + (size_t)h.row_bytes);
}
// The host twin of the inflate kernel: the kernel's algorithm (fl_inflate_core.h) in plain loops over arrays of the kernel's LDS sizes,
// on what png_stage_compressed left.  0 and scan[0 .. png_header_scan_bytes) = the scanlines, or kPngParse = the device's "no" (a
// caller then runs png_decode_scanlines, whose verdict is final), or kPngSmall.  stats: [0] blocks, [1] strips, [2] synchronisation
// rounds, [3] resolution rounds, [4] tokens decoded, [5] of those decoded more than once, [6] / [7] the most synchronisation / resolution
// rounds of one strip.
int png_inflate_model(const uint8_t *staged, size_t staged_bytes, uint8_t *scan, size_t cap, uint32_t stats[8]);

} // namespace fl
