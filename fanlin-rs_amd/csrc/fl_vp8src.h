// fl_vp8src.h -- host half of the lossy WebP decode front end (reference src/handler.rs:205-220: image 0.25.6 -> image-webp):
// the RIFF container, the VP8 key frame's headers, and the whole boolean-coded stage -- the first partition (segments, filter,
// quantisers, probability updates, every macroblock's modes) and the token partitions; for a compressed ALPH chunk also the
// lossless decoder's entropy stage (fl_webpsrc.cpp) on the headerless stream.  The serial stage runs here, on the
// calling thread; what it leaves -- one record per macroblock and the LEVELS, stored sparsely -- is what crosses PCIe, and the
// device (fl_vp8dec.hip) dequantises, transforms, predicts, filters and converts to RGB.  No HIP in this file or in
// fl_vp8src.cpp: with fl_webpsrc.cpp they compile alone with a plain C++ compiler (tests/vp8_src_fuzz.cpp).
//
// Refused with kVp8Unsupported (a well-formed file; the test corpus has no file with the feature that is checked against
// libwebp's decode, so it is not decoded):
//   - animation (ANIM / ANMF, or the VP8X animation flag)
//   - the colour-space bit or the clamping bit of the frame header set
//   - loop_filter_adj_enable with any non-zero ref_lf_delta / mode_lf_delta
//   - segment quantiser / filter values in delta mode
//   - a decoded picture of 2^31 bytes and more
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fl {

struct Vp8Info {
    uint32_t width = 0, height = 0;
    uint32_t channels = 0;          // of the picture the pipeline sees: 4 if the VP8X header announces alpha, else 3; 0 if unsupported
    uint32_t has_alpha = 0;         // the VP8X alpha flag
    uint32_t extended = 0;          // VP8X
    uint32_t animated = 0;          // VP8X animation flag, ANIM or ANMF
    uint32_t supported = 0;         // 1 = FLGPU_IMG_VP8_SOURCE decodes it
    uint32_t version = 0;           // of the frame tag (0..3)
    uint32_t segmentation = 0, update_map = 0;
    uint32_t filter_simple = 0, filter_level = 0, sharpness = 0;
    uint32_t partitions = 0;        // token partitions: 1, 2, 4 or 8
    uint32_t alpha_compression = 0, alpha_filter = 0; // of the ALPH chunk's first byte (0, 0 without one)
    uint32_t segment_quantizers = 0;    // different quantiser indices among the segments in use (1 without segmentation)
    uint32_t segment_filter_levels = 0; // different filter levels among them
    uint32_t coef_prob_updates = 0;     // coefficient probabilities the header replaces
    // deep parse only (the whole first partition and the token partitions are read)
    uint32_t macroblocks = 0, bpred_macroblocks = 0, skipped_macroblocks = 0;
    uint32_t skipped_bpred_macroblocks = 0; // skipped ones whose inner edges are filtered all the same
    uint32_t bmodes_mask = 0;       // bit k: sub-block mode k seen (numbered as in fl_vp8_dtables.h)
    uint32_t ymodes_mask = 0, uvmodes_mask = 0; // bit k: mode k seen (0 DC, 1 V, 2 H, 3 TM)
    uint32_t cat6_tokens = 0;
    uint32_t blob_bytes = 0;        // what vp8_decode_levels leaves for upload (Vp8BlobHeader::total_bytes)
    const char *refused = nullptr;  // supported == 0: the feature, for the error text
    size_t exif_off = 0, exif_len = 0; // the EXIF chunk's payload inside the file (0, 0: none)
    size_t vp8_off = 0, vp8_len = 0;   // the "VP8 " chunk's payload
    size_t alph_off = 0, alph_len = 0; // the ALPH chunk's payload (0, 0: none, or not wanted: no VP8X alpha flag)
};

// Return codes of the host half: 0 = ok, kVp8Parse = not a lossy WebP / damaged (FLGPU_ERR_PARSE), kVp8Unsupported = well-formed
// but not covered (FLGPU_ERR_UNSUPPORTED), kVp8Small = the caller's buffer is too small.
constexpr int kVp8Parse = -1, kVp8Unsupported = -2, kVp8Small = -3;

constexpr uint32_t kVp8BlobMagic = 0x31385056u; // "VP81"
constexpr uint64_t kVp8MaxDecoded = 1ull << 31;
constexpr uint32_t kVp8BPred = 4;               // Vp8MbRecord::ymode of a macroblock with sixteen sub-block modes

// What crosses PCIe: this header, the macroblock records (raster order), the levels, the ALPH payload.  Every offset is in bytes
// from the header's start and a multiple of 16.
struct alignas(16) Vp8BlobHeader {
    uint32_t magic;
    uint32_t width, height;   // of the decoded picture
    uint32_t channels;        // output channels: 3 or 4
    uint32_t mbw, mbh;
    uint32_t filter_type;     // 0 = none, 1 = simple, 2 = normal
    uint32_t alpha;           // 0: opaque (A = 255); 1 = the alpha plane at alpha_off, width x height bytes, filtered with alpha_filter;
                              // 2 = a lossless picture's blob there (fl_webpsrc.h, WebpBlobHeader first): the same plane in its green channel
    uint32_t alpha_filter;    // 0 none, 1 horizontal, 2 vertical, 3 gradient
    uint32_t rec_off, lev_off, alpha_off;
    uint32_t total_bytes;     // what is uploaded
    uint32_t nlevels;         // int16 levels stored behind lev_off
    uint32_t pad[2];
    uint16_t dq[4][8];        // per segment: y1 dc, y1 ac, y2 dc, y2 ac, uv dc, uv ac, 0, 0
};
static_assert(sizeof(Vp8BlobHeader) == 128, "blob header layout");

// One macroblock.  Blocks are numbered as the encoder numbers them (fl_vp8_core.h): 0..15 luma (raster), 16..19 U, 20..23 V, 24 Y2.
// Of block b the blob holds cnt[b] levels in coding (zig-zag) order, position 0 first -- up to the last non-zero one; the blocks
// of a macroblock follow each other from level index `lev`.
struct alignas(16) Vp8MbRecord {
    uint32_t lev;
    uint8_t ymode;            // 0 DC, 1 V, 2 H, 3 TM, kVp8BPred
    uint8_t uvmode;
    uint8_t segment;
    uint8_t inner;            // the loop filter runs on the inner edges: B_PRED, or any coefficient left after the transforms' input
    uint8_t f_limit, f_ilevel, hev_thresh, pad0; // f_limit == 0: this macroblock is not filtered
    uint8_t bmodes[8];        // sub-block b: (bmodes[b >> 1] >> 4 (b & 1)) & 15
    uint8_t cnt[25];
    uint8_t pad1[3];
};
static_assert(sizeof(Vp8MbRecord) == 48, "macroblock record layout");

// Container, frame tag, sizes and every header field of the first partition: allocates nothing.  deep = true also reads every
// macroblock's modes and all tokens (without storing them): the counts, the masks and blob_bytes.
int vp8_parse_info(const uint8_t *data, size_t n, Vp8Info &info, bool deep = false);

// Capacity to provide for vp8_decode_levels: the worst case of the blob.
size_t vp8_blob_capacity(const Vp8Info &info);

// Decodes a supported file into blob[0 .. cap) (16-byte aligned); hdr (optional) receives a copy of the header.  Nothing is
// allocated; every loop is bounded by the header's macroblock count.
int vp8_decode_levels(const uint8_t *data, size_t n, uint8_t *blob, size_t cap, Vp8BlobHeader *hdr);

} // namespace fl
