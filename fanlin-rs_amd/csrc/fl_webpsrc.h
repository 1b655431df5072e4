// fl_webpsrc.h -- host half of the lossless WebP decode front end (reference src/handler.rs:205-220: image 0.25.6 -> image-webp):
// the RIFF container, the VP8L headers, and the whole entropy stage -- prefix codes, LZ77, colour cache, every sub-image.
// The serial stage runs here, on the calling thread; what it leaves -- the RESIDUAL picture (one ARGB dword per pixel of the
// packed width) and the transforms' sub-images behind a small header -- is what crosses PCIe, and the device (fl_webpdec.hip)
// inverts the transforms.  No HIP in this file or in fl_webpsrc.cpp: both compile alone with a plain C++ compiler
// (tests/webp_host_fuzz.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fl {

struct WebpInfo {
    uint32_t width = 0, height = 0;
    uint32_t channels = 0;         // of the picture the pipeline sees: 4 if the file announces alpha, else 3; 0 if unsupported
    uint32_t has_alpha = 0;        // the VP8L header's alpha bit (simple form), the VP8X alpha flag (extended form)
    uint32_t extended = 0;         // VP8X
    uint32_t animated = 0;         // VP8X animation flag, ANIM or ANMF
    uint32_t lossless = 0;         // the picture is a VP8L chunk
    uint32_t transforms = 0;       // bit k = transform type k present (0 predictor, 1 cross-colour, 2 subtract-green, 3 colour indexing); deep parse only
    uint32_t color_cache_bits = 0; // of the main image; deep parse only
    uint32_t prefix_groups = 0;    // code groups of the main image; deep parse only
    uint32_t supported = 0;        // 1 = FLGPU_IMG_WEBP_SOURCE decodes it
    uint32_t blob_bytes = 0;       // what webp_decode_residuals will leave for upload (WebpBlobHeader::total_bytes); deep parse only
    size_t exif_off = 0, exif_len = 0; // the EXIF chunk's payload inside the file (0, 0: none)
    size_t vp8l_off = 0, vp8l_len = 0; // the VP8L chunk's payload
};

// Return codes of the host half: 0 = ok, kWebpParse = not a WebP / damaged (FLGPU_ERR_PARSE), kWebpUnsupported = well-formed
// but not covered (FLGPU_ERR_UNSUPPORTED), kWebpSmall = the caller's buffer is too small.
constexpr int kWebpParse = -1, kWebpUnsupported = -2, kWebpSmall = -3;

constexpr uint32_t kWebpMagic = 0x314c5057u; // "WPL1"
constexpr uint64_t kWebpMaxDecoded = 1ull << 31;

// transform types, as the stream numbers them
constexpr uint32_t kWtPredictor = 0, kWtCrossColor = 1, kWtSubtractGreen = 2, kWtColorIndexing = 3;

// What crosses PCIe in front of the sub-images and the residuals.  Every offset is in bytes from the header's start and a
// multiple of 16.
struct alignas(16) WebpBlobHeader {
    uint32_t magic;
    uint32_t width, height;   // of the decoded picture
    uint32_t channels;        // output channels: 3 (alpha dropped) or 4
    uint32_t ntransforms;
    uint32_t ttype[4];        // stream order; the device inverts them last to first
    uint32_t tbits[4];        // predictor / cross-colour: block bits 2..9; colour indexing: palette entries 1..256
    uint32_t twidth[4];       // the picture's width where this transform applies (packed if colour indexing came earlier in the stream)
    uint32_t toff[4];         // predictor: mode image; cross-colour: element image (both ceil(twidth / 2^bits) dwords a row);
                              // colour indexing: the palette, 256 dwords, entries beyond the file's 0x00000000
    uint32_t xsize;           // packed width: the residual picture is xsize x height dwords, a << 24 | r << 16 | g << 8 | b
    uint32_t res_off;
    uint32_t total_bytes;     // header + sub-images + residuals: what is uploaded
    uint32_t pad[4];
};
static_assert(sizeof(WebpBlobHeader) == 112, "blob header layout");

// pixels packed into one green byte by a palette of n entries: shift 3 / 2 / 1 / 0
inline uint32_t webp_index_shift(uint32_t n) { return n <= 2 ? 3u : n <= 4 ? 2u : n <= 16 ? 1u : 0u; }
inline uint32_t webp_subsample(uint32_t size, uint32_t bits) { return (size + (1u << bits) - 1u) >> bits; }

// Container, VP8L signature, sizes and alpha: allocates nothing, reads no entropy-coded data.  deep = true also walks the
// transform headers (decoding their sub-images into a work area of its own, bounded by the header's pixel count) and the
// main image's colour-cache and code-group header: transforms, color_cache_bits, prefix_groups.
int webp_parse_info(const uint8_t *data, size_t n, WebpInfo &info, bool deep = false);

// Capacity to provide for webp_decode_residuals: the blob itself (at most header + 3 sub-images + residuals) and behind it the
// decoder's work area (entropy image, code tables), which is not uploaded.
size_t webp_blob_capacity(const WebpInfo &info, size_t file_bytes);

// Entropy-decodes a supported file into blob[0 .. cap): header, sub-images, residuals; hdr (optional) receives a copy of the
// header.  Nothing is allocated; every loop is bounded by the header's pixel count.
int webp_decode_residuals(const uint8_t *data, size_t n, uint8_t *blob, size_t cap, WebpBlobHeader *hdr);

// The VP8L-coded alpha plane of a LOSSY picture's ALPH chunk (fl_vp8src.cpp): the stream without the five header bytes, width and
// height the frame's, the alpha values in the green channel.  The same blob (channels = 4), the same bounds; webp_alpha_blob_bytes
// says what webp_decode_alpha_residuals will leave (it reads the transform headers into a work area of its own).
size_t webp_alpha_blob_capacity(uint32_t width, uint32_t height, size_t stream_bytes);
int webp_decode_alpha_residuals(const uint8_t *data, size_t n, uint32_t width, uint32_t height, uint8_t *blob, size_t cap, WebpBlobHeader *hdr);
int webp_alpha_blob_bytes(const uint8_t *data, size_t n, uint32_t width, uint32_t height, uint32_t *bytes);

} // namespace fl
