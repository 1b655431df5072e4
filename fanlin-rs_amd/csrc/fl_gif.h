// fl_gif.h -- the GIF encoder (fl_gif.hip): job descriptor, segment geometry and the format's worst case.
// What image 0.25.6's GifEncoder::encode_frames writes for frames of at most 256 colours (gif 0.13.1, Frame::from_rgba_speed's
// exact-palette branch): every frame a full-canvas image with a local colour table, disposal 1, delay 0, an endless loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_gif_quant_core.h"

namespace fl {

// A frame's indices are LZW-coded in independent segments of kGifSegIndices: each one starts from an empty table and closes
// with a clear code (the frame's last one with the end code), so no segment's code widths depend on anything outside it.
// At most 3,838 (4,096 - 258 entries at code size 8) keeps the table from ever filling: no code is written at a full table.
constexpr uint32_t kGifSegIndices = 2048;
constexpr uint32_t kGifSegDwords = 772;    // scratch of one segment: (kGifSegIndices + 2) codes of 12 bits = 769 dwords, rounded up
constexpr uint32_t kGifColourSlots = 1024; // open-addressing table of a frame's colours (at most 256 + one per thread in flight)
constexpr uint32_t kGifDictSlots = 4096;   // open-addressing LZW dictionary of a segment (at most kGifSegIndices - 1 entries)
constexpr uint32_t kGifThreads = 256;
constexpr uint32_t kGifFileHead = 32;      // "GIF89a" + logical screen (13) and the NETSCAPE2.0 block (19)
constexpr uint32_t kGifFrameRec = 8;       // dwords of a frame's record, below
static_assert(kGifSegIndices <= 3838, "a segment must not be able to fill the LZW table");
static_assert((uint64_t)(kGifSegIndices + 2) * 12 <= (uint64_t)(kGifSegDwords - 2) * 32, "segment scratch too small");

// frame record words
enum { kGrColours = 0, kGrTableBits = 1, kGrCodeSize = 2, kGrTransparent = 3, kGrHeadBytes = 4, kGrDataBits = 5, kGrBytes = 6,
       kGrQuant = 7 /* 0 = exact palette; else the quantiser's mark, s and clear bit (fl_gif_quant_core.h) */ };
constexpr uint32_t kGifNoTransparent = 0xffffffffu;

inline uint64_t gif_segments(uint64_t pixels) { return (pixels + kGifSegIndices - 1) / kGifSegIndices; }
// The LZW data of one frame at its worst: a clear code in front, one code per index and every segment's closing code, all at 12 bits.
inline uint64_t gif_max_data_bytes(uint64_t pixels) { return (12u * (pixels + 1u + gif_segments(pixels)) + 7u) / 8u; }
// The format's worst case for one frame: graphic control extension 8 + image descriptor 10 + local table 768 + code size 1 +
// the data in sub-blocks of 255 (a length byte each) + the terminator.
inline uint64_t gif_max_frame_bytes(uint64_t pixels)
{
    const uint64_t d = gif_max_data_bytes(pixels);
    return 8u + 10u + 768u + 1u + d + (d + 254u) / 255u + 1u;
}
// What a destination has to hold for either outcome (the file, or the frames' pixels): 64 + frames x max(pixel bytes, worst frame).
inline uint64_t gif_max_file_bytes(uint64_t frames, uint64_t frame_max) { return 64u + frames * frame_max; }

// What the encoder takes: LumaA8 or Rgba8 frames whose sides fit the logical screen's 16 bits, and a file whose bit and byte
// offsets fit 32 bits with room to spare.  Anything else leaves as pixels, as without FLGPU_ENCODE_GIF.
inline bool gif_encodable(uint64_t w, uint64_t h, uint32_t c, uint64_t frames, uint64_t pixel_bytes)
{
    if ((c != 2u && c != 4u) || !w || !h || w > 65535u || h > 65535u || !frames || frames > 65535u) return false;
    const uint64_t px = w * h;
    return px <= (1ull << 27) && gif_max_file_bytes(frames, gif_max_frame_bytes(px) > pixel_bytes ? gif_max_frame_bytes(px) : pixel_bytes) < (1ull << 31);
}

// The quantiser's cells of one frame: the hash slots of s = 0, 1, 2, or the direct table of s = 3, which takes more than
// kGifQuantHashCells colours and so as many pixels.
inline uint32_t gif_quant_stride(uint64_t pixels) { return pixels > kGifQuantHashCells ? kGifQuantCells : kGifQuantHashSlots; }
// What a file may ask of the quantiser: frames of at most kGifQuantMaxPixels (the 64-bit products) and at most 1 GiB of cells
// (20 bytes a cell and frame).  A file beyond either is treated as without FLGPU_ENCODE_GIF_QUANTIZE.
inline bool gif_quantizable(uint64_t pixels, uint64_t frames) { return pixels <= kGifQuantMaxPixels && frames * gif_quant_stride(pixels) * 20u <= (1ull << 30); }

// One animation of a GIF-encode launch: `frames` pictures of w x h pixels with c = 2 (LumaA8) or 4 (Rgba8) channels.
struct GifEncJob {
    const uint8_t *pixels;   // frame f at pixels + f * pix_pitch (256-byte aligned)
    uint64_t pix_pitch;
    uint32_t *status;        // [0] = a frame has more than 256 colours and is not quantised (nothing else is valid then), [1] = file bytes,
                             // [2] = frames the quantiser gave their table
    uint32_t *frec;          // [frame][kGifFrameRec]
    uint32_t *ckeys, *cvals; // [frame][kGifColourSlots] colour -> index, as the palette kernel's hash left it
    uint8_t *indices;        // frame f at indices + f * idx_pitch
    uint32_t *segs;          // [frame * nseg + segment][kGifSegDwords] the segment's codes
    uint32_t *seg_bits;      // [frame * nseg + segment] bits of them
    uint32_t *seg_off;       // [frame * nseg + segment] bits of the frame's segments in front of it
    uint8_t *bodies;         // frame f's blocks (control extension .. terminator) at bodies + f * body_pitch
    uint8_t *file;           // the finished file
    uint64_t idx_pitch, body_pitch;
    uint32_t w, h, c, frames;
    uint32_t px, nseg;       // pixels and segments of one frame
    // FLGPU_ENCODE_GIF_QUANTIZE (fl_gifquant.hip): quant != 0 marks a frame above 256 colours instead of the file.  Per frame
    // 4 x qstride words of cells (n, sum r, sum g, sum b, an array each) and qstride words box << 24 | representative.
    uint32_t quant, qstride;
    uint32_t *qcells, *qbox;
};

// palette -> indices -> LZW segments -> scan -> pack -> file; six stream-ordered launches, nothing waits between workgroups
// (with job.quant three more behind the palette kernel: cells -> split -> nearest entry, launch_gif_quantize)
hipError_t launch_gif_encode(const GifEncJob &job, hipStream_t st);
void launch_gif_quantize(const GifEncJob &job, hipStream_t st);

} // namespace fl
