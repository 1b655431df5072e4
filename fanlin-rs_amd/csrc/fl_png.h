// fl_png.h -- the PNG encoder (fl_png.hip): job descriptor, segment geometry and the format's worst case.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fl {

// The filtered stream (h rows of 1 filter byte + w * c bytes) is deflated in independent segments of kPngSegBytes; each one
// sees the kPngSegBytes before it as history, ends on a byte boundary and becomes one IDAT chunk.
constexpr uint32_t kPngSegBytes = 32768;
constexpr uint32_t kPngSegOutBytes = kPngSegBytes + 256; // chunk scratch per segment: 12 chunk bytes + 2 zlib header + 5 + data
constexpr uint32_t kPngThreads = 256;

// One picture of a PNG-encode launch.
struct alignas(16) PngJob {
    const uint8_t *src;   // interleaved pixels, w x h x c
    uint8_t *dst;         // the PNG file
    uint8_t *filt;        // scratch: h x (1 + w c) filtered rows (256-byte aligned)
    uint8_t *chunks;      // scratch: [segment][kPngSegOutBytes] the segment's IDAT chunk
    uint16_t *syms;       // scratch: [segment][kPngSegBytes] LZ77 symbols
    uint32_t *recs;       // scratch: [segment][4] chunk bytes, Adler-32 A and B of the segment, segment bytes
    uint32_t *result;     // [1] = stream bytes (0 if it did not fit dst_cap): the words and protocol of JpegJob
    uint32_t w, h, c;
    uint32_t row0, seg0;  // first row / segment of the picture in the launch's flat row / segment numbering
    uint32_t nseg;
    uint32_t level;       // 0 = Fast, 1 = Default, 2 = Best
    uint32_t dst_cap;     // bytes available at dst
    uint64_t fbytes;      // filtered bytes
};

// quality -> compression level, reference src/handler.rs:264-273 (unclamped): < 50 Best, < 85 Default, otherwise Fast
inline uint32_t png_level(uint32_t quality) { return quality < 50u ? 2u : quality < 85u ? 1u : 0u; }

inline uint64_t png_filtered_bytes(uint64_t w, uint64_t h, uint64_t c) { return h * (1u + w * c); }
inline uint64_t png_segments(uint64_t fbytes) { return (fbytes + kPngSegBytes - 1) / kPngSegBytes; }

// The format's worst case: every segment as stored blocks (5 bytes per block of <= 65,535) plus its sync flush (5) and chunk
// framing (12); signature 8 + IHDR 25 + zlib header 2 + Adler-32 4 with its own chunk 12 + IEND 12.
inline uint64_t png_max_out_bytes(uint64_t fbytes)
{
    const uint64_t nseg = png_segments(fbytes), full = nseg - 1, last = fbytes - full * kPngSegBytes;
    auto seg = [](uint64_t l) { return l + 5u * ((l + 65534u) / 65535u) + 5u + 12u; };
    return 8u + 25u + 2u + 4u + 12u + 12u + full * seg(kPngSegBytes) + seg(last);
}

// filter rows -> deflate segments -> frame the file; three stream-ordered launches
hipError_t launch_png_encode(const PngJob *jobs, uint32_t njobs, uint32_t total_rows, uint32_t total_segs, hipStream_t st);

} // namespace fl
