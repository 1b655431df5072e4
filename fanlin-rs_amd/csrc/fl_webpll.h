// fl_webpll.h -- the lossless WebP encoder (fl_webpll.hip): job descriptor, tile geometry and the format's worst case.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fl {

// A picture's pixels are cut into tiles of kWebpllTile in raster order; per-tile launches take one tile per workgroup, per-picture
// launches one picture.
constexpr uint32_t kWebpllTile = 4096;
constexpr uint32_t kWebpllThreads = 256;
constexpr uint32_t kWebpllMaxSide = 16384;  // the VP8L header holds 14 bits of width - 1 and of height - 1
// per-picture scratch words: four histograms, the four codes (length << 16 | reversed code), the header bits, counters
constexpr uint32_t kWebpllPicWords = 2432;

// A tile's record: the tile's last run start (index + 1, 0 = none), the one carried into it, its data bits and their offset.
struct WebpllTile {
    uint32_t last, carry, bits, pad;
    uint64_t off, pad2;
};

// What a job's stream is for.  A launch's jobs share one mode: the kernels are instantiated per mode.
//   file   the finished RIFF / VP8L file of the picture's pixels at dst (FLGPU_FE_WEBP_LOSSLESS).
//   alpha  the ALPH payload of a lossy WebP file (FLGPU_FEO_ALPHA_VP8L): the pixels are ARGB (255, 0, a, 0) of an alpha plane, the
//          stream has no VP8L header and no subtract-green transform, nothing is framed.  A picture whose result[0] has bit 0
//          clear (the planes launch found it opaque) is left alone: every workgroup returns after reading that word.
enum : uint32_t { kWebpllModeFile = 0, kWebpllModeAlpha = 1 };

// One picture of a lossless-WebP launch.
struct alignas(16) WebpJob {
    const uint8_t *src;   // file: interleaved pixels, w x h x c; alpha: the plane, w x h bytes
    uint8_t *dst;         // file: the WebP file; alpha: the coder's result -- a word with the stream's bytes (0: it did not fit
                          // the scratch), the byte-aligned stream from byte kWebpllAlphaHead on (= stream)
    uint32_t *res;        // scratch: [w h] residuals, ARGB (256-byte aligned)
    uint16_t *tok;        // scratch: [w h] tokens: 0x8000 literal, 1..4096 a backward reference of that length ends here, 0 none
    WebpllTile *tiles;    // scratch: [ntiles]
    uint32_t *pic;        // scratch: [kWebpllPicWords]
    uint32_t *stream;     // scratch: the VP8L bit stream, from the signature byte on (webpll_max_out_bytes bytes)
    uint32_t *result;     // [1] = file bytes (0 if it did not fit dst_cap): the words and protocol of JpegJob; alpha: the lossy job's
                          // words, of which only bit 0 of [0] is read
    uint32_t w, h, c;
    uint32_t tile0;       // first tile of the picture in the launch's flat tile numbering
    uint32_t ntiles;
    uint32_t dst_cap;     // bytes available at dst
    uint32_t stream_words; // words at stream
    uint32_t mode;        // kWebpllModeFile / kWebpllModeAlpha
};
static_assert(sizeof(WebpJob) == 96, "the job record: the mode took the spare word");
constexpr uint32_t kWebpllAlphaHead = 16; // bytes in front of an alpha job's stream: the byte count and padding to a 16-byte boundary

inline uint64_t webpll_tiles(uint64_t npix) { return (npix + kWebpllTile - 1u) / kWebpllTile; }

// The format's worst case.  A literal costs at most 4 x 15 bits (four codes of at most 15 bits).  A backward reference costs at
// most 15 + 10 bits (length code + extra bits; the distance code has one symbol, 0 bits) and always follows a literal, so a pixel
// never costs more than 60 bits.  Everything in front of the pixel data -- RIFF and chunk headers (20 bytes), the 40 header
// bits, the transforms and their sub-image (37), 3 flag bits, the green code (at most 1 + 4 + 57 + 1 + 280 x 7 bits), three
// 256-symbol codes (at most 1 + 4 + 57 + 12 + 256 x 7 bits each), the distance code (4) and the pad byte -- comes to at most
// 20 + 964 + 1 bytes.  Hence 1024 + ceil(15 w h / 2).
inline uint64_t webpll_max_out_bytes(uint64_t w, uint64_t h) { return 1024u + (15u * w * h + 1u) / 2u; }

// residuals -> run starts carried across tiles -> tokens and histograms -> codes and header -> bits per tile -> offsets ->
// bits placed -> the file (alpha: the byte count); eight stream-ordered launches of the mode's instantiations
hipError_t launch_webpll_encode(const WebpJob *jobs, uint32_t njobs, uint32_t total_tiles, hipStream_t st, uint32_t mode = kWebpllModeFile);

} // namespace fl
