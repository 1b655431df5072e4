// fl_gifsrc.h -- host half of the GIF decode front end (reference src/handler.rs:311-366, process_gif: image 0.25.6 -> gif):
// the container (logical screen, colour tables, graphic control extensions, image descriptors, data sub-blocks) and the whole
// LZW stage.  The serial stage runs here, on the calling thread; what it leaves -- one record and the INDEX bytes of every
// frame in stored row order, and one 256-entry palette per colour table, behind a small header -- is what crosses PCIe, and
// the device (fl_gifdec.hip) looks the colours up, undoes the interlace and walks the disposal chain.  No HIP in this file or
// in fl_gifsrc.cpp: both compile alone with a plain C++ compiler (tests/gif_host_fuzz.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fl {

struct GifInfo {
    uint32_t width = 0, height = 0;   // the logical screen = the canvas every frame is composited onto
    uint32_t frames = 0;
    uint32_t has_global_table = 0;
    uint32_t interlaced_frames = 0;
    uint32_t transparent_frames = 0;  // frames whose graphic control extension names a transparent index
    uint32_t disposal_mask = 0;       // bit k = disposal method k occurs
    uint32_t max_code_size = 0;       // the largest LZW minimum code size of a frame
    uint64_t decoded_bytes = 0;       // frames x width x height x 4
    uint32_t supported = 0;           // 1 = the container holds nothing the decoder does not vouch for (the LZW stage may still say otherwise)
    uint64_t index_bytes = 0;         // sum of the frames' w x h
};

// Return codes of the host half: 0 = ok, kGifParse = not a GIF / damaged (FLGPU_ERR_PARSE), kGifUnsupported = well-formed but
// not vouched for (FLGPU_ERR_UNSUPPORTED), kGifSmall = the caller's buffer is too small.
constexpr int kGifParse = -1, kGifUnsupported = -2, kGifSmall = -3;

constexpr uint32_t kGifMagic = 0x31464947u;        // "GIF1"
constexpr uint32_t kGifMaxFrames = 4096;
constexpr uint64_t kGifMaxDecoded = 512ull << 20;  // frames x width x height x 4: the JPEG decoder's cap on decoded bytes

// What crosses PCIe: header, frame records, index bytes, palettes.  Every offset is in bytes from the header's start; the
// first frame's indices and the palettes start at multiples of 16.
struct alignas(16) GifBlobHeader {
    uint32_t magic;
    uint32_t width, height;   // of the canvas
    uint32_t frames;
    uint32_t palettes;        // 1,024-byte palettes stored
    uint32_t pal_off;         // the first palette (the frame records start at sizeof(GifBlobHeader))
    uint32_t idx_off;         // the first frame's index bytes
    uint32_t total_bytes;     // what is uploaded
};
static_assert(sizeof(GifBlobHeader) == 32, "blob header layout");

struct alignas(16) GifFrameRec {
    uint32_t x, y, w, h;      // the frame's rectangle, inside the canvas
    uint32_t disposal;        // 0..7 as the file says
    uint32_t interlaced;
    uint32_t pal_off;         // this frame's palette: 256 dwords R | G << 8 | B << 16 | 255 << 24; entries beyond the table's size 0;
                              // the transparent index, if the frame has one, 0 (then the palette is a copy of the frame's own)
    uint32_t idx_off;         // w x h index bytes, rows in the order the file stores them
};
static_assert(sizeof(GifFrameRec) == 32, "frame record layout");

// The container alone, to the trailer: allocates nothing, skips the LZW data.  kGifParse for a damaged file; supported = 0
// for one the decoder does not vouch for.
int gif_parse_info(const uint8_t *data, size_t n, GifInfo &info);

// Capacity to provide for gif_decode_blob (the palette count is known only after the walk: one per frame and the global one
// bound it).
size_t gif_blob_capacity(const GifInfo &info);

// Describes the file, then walks it once more and LZW-decodes every frame into blob[0 .. cap): header, records, indices, palettes; hdr (optional)
// receives a copy of the header.  Nothing is allocated; every loop is bounded by the file's length or a frame's w x h.
int gif_decode_blob(const uint8_t *data, size_t n, uint8_t *blob, size_t cap, GifBlobHeader *hdr);

} // namespace fl
