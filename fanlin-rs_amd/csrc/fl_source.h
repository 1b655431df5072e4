// fl_source.h -- encoded files on the way into a batch:
//   fl_source.cpp    JPEG / PNG / lossless WebP / lossy WebP files as SOURCES of a batch: probe (header + what the caller announced), stage (the host
//                    half, into the caller's staging), decode (the device half, in front of run_batch_device)
//   fl_gifrun.cpp    a GIF file, which is no source of a batch but a batch of its own (a caller of run_batch_device)
// The per-format host decoders are fl_jpeghuff.cpp, fl_pngsrc.cpp, fl_webpsrc.cpp, fl_vp8src.cpp and fl_gifsrc.cpp; they know nothing of contexts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/fanlin_gpu.h"
#include "fl_gifdec.h"
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

// What source_probe learns from a source before anything is reserved for it.
struct SourceProbe {
    SourceKind kind = SRC_PIXELS;
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
    PngBlobHeader png;        // SRC_PNG: header + filtered scanlines the staging thread inflated
    WebpBlobHeader webp;      // SRC_WEBP: header + sub-images + residuals the staging thread entropy-decoded
    Vp8BlobHeader vp8;        // SRC_VP8: header + macroblock records + levels (+ ALPH payload) the staging thread decoded
    WebpBlobHeader vp8_alpha; // ... vp8.alpha == 2: the header of the lossless blob that holds the alpha plane
    uint64_t file_bytes = 0;  // of the file (the *_file_bytes counters)
    size_t used = 0;          // bytes of the staging to upload
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

// ---- fl_gifrun.cpp ---------------------------------------------------------------------------------------------------
// A GIF file (not a source of a batch: it IS one).  The LZW stage runs on the calling thread, outside the context's lock; then blob
// upload, gif_compose_kernel into scratch, and -- with params -- the frames as one device-resident Rgba8 batch with the same
// params through run_batch_device: dst->data receives *frames results plan.out_bytes apart.  params == nullptr: the composited
// frames themselves.  With FLGPU_ENCODE_GIF in accept_flags the encoder (fl_gif.hip) runs behind the batch and dst receives the
// finished file, or -- a frame above 256 colours -- the same pixels; *result_kind says which.
int run_gif_host(flgpu_ctx *c, const uint8_t *gif, size_t n, const flgpu_params *params, uint32_t accept_flags, flgpu_image *dst, uint32_t *frames, int *result_kind);

} // namespace fl
