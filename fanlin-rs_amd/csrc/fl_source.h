// fl_source.h -- encoded files on the way into a batch:
//   fl_request.cpp   a file + query string + accept flags as ONE request (the flgpu_process_* / flgpu_decode_* / flgpu_*_info_of entry points): head,
//                    plan, run -- whatever the format
//   fl_source.cpp    JPEG / PNG / lossless WebP / lossy WebP files as SOURCES of a batch: probe (header + what the caller announced), stage (the host
//                    half, into the caller's staging), decode (the device half, in front of run_batch_device)
//   fl_gifrun.cpp    a GIF file, which is no source of a batch but a batch of its own (a caller of run_batch_device)
// The per-format host decoders are fl_jpeghuff.cpp, fl_pngsrc.cpp, fl_webpsrc.cpp, fl_vp8src.cpp and fl_gifsrc.cpp; they know nothing of contexts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/fanlin_gpu.h"
#include "fl_gifdec.h"
#include "fl_inflate.h"
#include "fl_jpegdec.h"
#include "fl_pngdec.h"
#include "fl_vp8dec.h"
#include "fl_webpdec.h"

namespace fl {

// What flgpu_image::flags announce; where several are set: JPEG, then PNG, then lossless WebP, then lossy WebP.
enum SourceKind : uint32_t { SRC_PIXELS = 0, SRC_JPEG, SRC_PNG, SRC_WEBP, SRC_VP8 };
inline SourceKind source_kind(uint32_t flags)
{
    return (flags & FLGPU_IMG_JPEG_SOURCE) ? SRC_JPEG : (flags & FLGPU_IMG_PNG_SOURCE) ? SRC_PNG : (flags & FLGPU_IMG_WEBP_SOURCE) ? SRC_WEBP
           : (flags & FLGPU_IMG_VP8_SOURCE) ? SRC_VP8 : SRC_PIXELS;
}

// What a request needs of a file's header, whatever the format (file_head below fills it).
struct FileHead {
    uint32_t width = 0, height = 0;
    uint32_t channels = 0;    // of the decoded picture; 0 if unsupported -- but a JPEG announces 1 (one component) or 3 either way: it is planned before it is refused
    uint32_t flags = 0;       // what a flgpu_image of the file carries: FLGPU_IMG_*_SOURCE (| FLGPU_IMG_PNG_ADAM7)
    int input_format = 0;     // FLGPU_IN_*; both WebP kinds are FLGPU_IN_WEBP
    uint32_t orientation = 0; // EXIF, 1..8; 0 = no tag (a request then runs with 1).  The PNG decoder reports none (handler.rs:206): always 0
    uint32_t supported = 0;   // 1 = the device decoder takes the file
};

// What source_probe learns from a source before anything is reserved for it.
struct SourceProbe {
    SourceKind kind = SRC_PIXELS;
    FileHead head;       // of a file (file_head)
    size_t capacity = 0; // of the buffer source_stage fills: jpeg_source_capacity / png_blob_bytes / webp_blob_capacity / vp8_blob_capacity, or W*H*C for pixels
    JpegInfo jpeg;       // the header of `kind`
    PngInfo png;
    WebpInfo webp;
    Vp8Info vp8;
};

// One source as it goes to the device: for a file the host copy of its blob header (the blob itself is in the staging that source_stage
// filled), for pixels nothing but the kind.  One per image of a host batch, one inside every queued Request.
struct StagedSource {
    SourceKind kind = SRC_PIXELS;
    JpegBlobHeader jpeg;      // SRC_JPEG: the coefficient blob the staging thread decoded, or ...
    JpegHuffStage stage{};    // ... jpeg.magic == kJhMagic: the staged entropy-coded segment, decoded on the device (a host copy of its description)
    std::vector<uint8_t> icc; // four-component JPEG + use_embedded_profile: the file's own ICC profile
    PngBlobHeader png;        // SRC_PNG: header + filtered scanlines the staging thread inflated, or (magic kPngzMagic) header + the deflate stream for the device
    WebpBlobHeader webp;      // SRC_WEBP: header + sub-images + residuals the staging thread entropy-decoded
    Vp8BlobHeader vp8;        // SRC_VP8: header + macroblock records + levels (+ ALPH payload) the staging thread decoded
    WebpBlobHeader vp8_alpha; // ... vp8.alpha == 2: the header of the lossless blob that holds the alpha plane
    uint64_t file_bytes = 0;  // of the file (the *_file_bytes counters)
    size_t used = 0;          // bytes of the staging to upload
};

// The header of a file of `kind`, into out.kind / out.head / that kind's *Info: the ONE place outside the per-format decoders that parses a header for a
// request, a source or an info call.  0, or FLGPU_ERR_PARSE.  Depth: the layout alone (requests and sources: flgpu_transform verifies CRCs and reads
// the streams once, under the decode bound; as_is serves the file unread) unless HEAD_FULL (the *_info_of calls: PNG CRCs, the WebP streams' contents).
// HEAD_SNIFF: a SRC_WEBP file whose picture is a `VP8 ` chunk becomes SRC_VP8 (flgpu_process_webp goes by the chunk type; a source goes by its flag).
// HEAD_INFLATE: a PNG head carries FLGPU_IMG_PNG_INFLATE (the request asked for the device inflate); what the head reports is the same.
enum : uint32_t { HEAD_ADAM7 = 1u, HEAD_FULL = 2u, HEAD_SNIFF = 4u, HEAD_INFLATE = 8u };
// the HEAD_* options the flags of a PNG source stand for
inline uint32_t png_head_opts(uint32_t src_flags) { return ((src_flags & FLGPU_IMG_PNG_ADAM7) ? HEAD_ADAM7 : 0u) | ((src_flags & FLGPU_IMG_PNG_INFLATE) ? HEAD_INFLATE : 0u); }
int file_head(SourceKind kind, const uint8_t *file, size_t n, uint32_t opts, SourceProbe &out);
// the flgpu_image a file with that head is handed over as
inline flgpu_image file_image(const uint8_t *file, uint64_t n, const FileHead &h)
{
    flgpu_image src;
    memset(&src, 0, sizeof(src));
    src.data = const_cast<uint8_t *>(file); src.capacity = n;
    src.width = h.width; src.height = h.height; src.channels = h.channels; src.flags = h.flags;
    return src;
}

// A host buffer of `cap` bytes that starts at a multiple of 16, as the staging flgpu_transform decodes a blob into does.
struct WorkBuf {
    std::unique_ptr<uint8_t[]> mem;
    uint8_t *p;
    explicit WorkBuf(size_t cap) : mem(new uint8_t[cap + 16u]), p(mem.get() + ((16u - (reinterpret_cast<uintptr_t>(mem.get()) & 15u)) & 15u)) {}
};

// Decides the kind and holds the file against what the caller announced: that format's header parse, width / height / channels, for JPEG
// the precheck below, for pixels capacity >= W*H*C.  Runs BEFORE anything is reserved on the file's say-so.  FLGPU_ERR_INVALID_ARG for a JPEG
// that does not parse, FLGPU_ERR_PARSE for PNG / WebP (lossless and lossy); a JPEG the device path does not cover is FLGPU_ERR_UNSUPPORTED without an error text.
int source_probe(flgpu_ctx *c, const flgpu_image *src, SourceProbe &out);
// The host half of a file source: decodes (or, JPEG, only stages) `src` into buf[0 .. cap), cap >= probe.capacity, and describes the result in
// `out`.  Takes the ICC profile out of `probe` where the decode will need it.  host_huffman: a JPEG is Huffman-decoded here in any case.
int source_stage(flgpu_ctx *c, const flgpu_image *src, SourceProbe &probe, void *buf, size_t cap, StagedSource &out, bool host_huffman = false);
// The device half for a batch: dsrc[i].data = DEVICE copy of what source_stage left for staged[i] (untouched for pixels).  Runs the JPEG, PNG,
// WebP and lossy WebP decode kernels into scratch, points dsrc[i] at the pixels, and advances the sources' counters.
int decode_sources(flgpu_ctx *c, size_t n, flgpu_image *dsrc, const StagedSource *const *staged, hipStream_t st);

// After the batch decode_sources fed has completed on `st`: bad[i] = 1 where the device entropy decoder gave up on picture i
// (its states did not settle, or the stream holds an invalid code word): the caller decodes that file on the host instead.
// Returns the number of such pictures, or a negative FLGPU_ERR_* .
int entropy_failures(flgpu_ctx *c, size_t n, std::vector<uint8_t> &bad, hipStream_t st, bool fetched = false);
int entropy_failures_fetch(flgpu_ctx *c, size_t n, hipStream_t st);
// internal status of a queued request: run it again with the host entropy decoder
constexpr int FL_STATUS_RETRY_HOST_HUFFMAN = 1000;
// set while a request is run again after the device entropy decoder gave up on its file (this thread's JPEG sources are then decoded on the host)
extern thread_local bool tl_force_host_huffman;
struct ForceHostHuffman { // the guard around such a second run; active(): this thread is inside one (a second failure is final)
    ForceHostHuffman() { tl_force_host_huffman = true; }
    ~ForceHostHuffman() { tl_force_host_huffman = false; }
    static bool active() { return tl_force_host_huffman; }
};
int device_huffman_policy(const flgpu_ctx *c, uint64_t file_bytes);

inline int gif_status(int rc) { return rc == 0 ? FLGPU_OK : rc == kGifParse ? FLGPU_ERR_PARSE : rc == kGifUnsupported ? FLGPU_ERR_UNSUPPORTED : FLGPU_ERR_BUFFER_TOO_SMALL; }
inline int vp8_status(int rc) { return rc == 0 ? FLGPU_OK : rc == kVp8Parse ? FLGPU_ERR_PARSE : rc == kVp8Unsupported ? FLGPU_ERR_UNSUPPORTED : FLGPU_ERR_BUFFER_TOO_SMALL; }
inline int webp_status(int rc) { return rc == 0 ? FLGPU_OK : rc == kWebpParse ? FLGPU_ERR_PARSE : rc == kWebpUnsupported ? FLGPU_ERR_UNSUPPORTED : FLGPU_ERR_BUFFER_TOO_SMALL; }
inline int png_status(int rc) { return rc == 0 ? FLGPU_OK : rc == kPngParse ? FLGPU_ERR_PARSE : rc == kPngUnsupported ? FLGPU_ERR_UNSUPPORTED : FLGPU_ERR_BUFFER_TOO_SMALL; }

// The device's Y | U | V planes of a lossy WebP file (padded to whole macroblocks, vp8_rec_bytes), before (filter == 0) or behind
// the loop filter: what flgpu_debug_vp8_planes hands out, so that a wrong pixel names its stage.  Buffers of its own, no batch.
int debug_vp8_planes(flgpu_ctx *c, const uint8_t *file, size_t n, int filter, uint8_t *out, size_t capacity, size_t *used);
// The scanlines of a PNG file exactly as the inflate kernel leaves them: buffers of its own, no batch, no host re-run (a device "no" is
// FLGPU_ERR_PARSE).  What flgpu_debug_png_inflate_device hands out, so that a wrong pixel names its stage.
int debug_png_inflate_device(flgpu_ctx *c, const uint8_t *file, size_t n, uint32_t src_flags, uint8_t *out, size_t capacity, size_t *used);

// ---- fl_query.cpp: the planner behind every request -----------------------------------------------------------------------
// Everything State::process_image decides before it touches pixels (handler.rs:198-261).
int plan_request(const flgpu_image *decoded, uint8_t exif_orientation, const char *query_string, uint32_t accept_flags, int input_format,
                 flgpu_params *p, flgpu_plan *plan, int *result_kind, int *out_format);
// A file the device decoder does not take: only as_is, which never decodes, gets through (verdict order: query parse, size gate, as_is; the plan zeroed).
int plan_undecodable(const char *query_string, flgpu_plan *plan, int *kind, int *out_format);
// The shared end of flgpu_process_{image,jpeg,png,webp}: rc and kind are the planner's verdict; as_is never reaches the device.
int run_planned(flgpu_ctx *ctx, int rc, int kind, int *result_kind, const flgpu_image *src, const flgpu_params *p, flgpu_image *dst);

// ---- fl_gifrun.cpp ---------------------------------------------------------------------------------------------------
// A GIF file (not a source of a batch: it IS one).  The LZW stage runs on the calling thread, outside the context's lock; then blob
// upload, gif_compose_kernel into scratch, and -- with params -- the frames as one device-resident Rgba8 batch with the same
// params through run_batch_device: dst->data receives *frames results plan.out_bytes apart.  params == nullptr: the composited
// frames themselves.  With FLGPU_ENCODE_GIF in accept_flags the encoder (fl_gif.hip) runs behind the batch and dst receives the
// finished file, or -- a frame above 256 colours -- the same pixels; *result_kind says which.
int run_gif_host(flgpu_ctx *c, const uint8_t *gif, size_t n, const flgpu_params *params, uint32_t accept_flags, flgpu_image *dst, uint32_t *frames, int *result_kind);

} // namespace fl
