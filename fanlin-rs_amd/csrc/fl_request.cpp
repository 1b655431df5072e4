// fl_request.cpp -- file bytes + query string + accept flags as one request (fl_source.h): what the headers say (flgpu_*_info_of), the one
// planner and runner behind flgpu_process_{jpeg,png,webp}[_plan], the one decoder entry behind flgpu_decode_*, the host halves alone
// (flgpu_debug_*_blob and their kin), and GIF files, which are a batch of their own.  No device code.
#include <string.h>

#include <algorithm>

#include "fl_context.h" // (the runtime's other headers come with it)

using fl::SourceKind;

/* One file request up to its verdict: *src is the file as a source, the rest is as plan_request leaves it. */
static int plan_file(SourceKind kind, const uint8_t *file, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_image *src,
                     flgpu_params *p, flgpu_plan *plan, int *result_kind, int *out_format)
{
    if (!file) return FLGPU_ERR_INVALID_ARG;
    /* FLGPU_DECODE_PNG_ADAM7 in the accept flags becomes FLGPU_IMG_PNG_ADAM7 on the source */
    const uint32_t adam7 = kind != fl::SRC_PNG ? 0u : ((accept_flags & FLGPU_DECODE_PNG_ADAM7) ? fl::HEAD_ADAM7 : 0u) |
                           ((accept_flags & FLGPU_DECODE_PNG_INFLATE) ? fl::HEAD_INFLATE : 0u); /* ... and FLGPU_DECODE_PNG_INFLATE becomes FLGPU_IMG_PNG_INFLATE */
    fl::SourceProbe probe;
    if (int rc = fl::file_head(kind, file, (size_t)n, fl::HEAD_SNIFF | adam7, probe)) return rc;
    const fl::FileHead &h = probe.head;
    *src = fl::file_image(file, n, h);
    /* a JPEG alone is planned BEFORE it is refused: a query or geometry error wins over FLGPU_ERR_UNSUPPORTED and the plan is filled.  The others
       (the canvas may be beyond what a plan can describe): plan_undecodable's order -- query parse, size gate, as_is -- and a zeroed plan */
    if (!h.supported && probe.kind != fl::SRC_JPEG) return fl::plan_undecodable(query_string, plan, result_kind, out_format);
    /* ImageDecoder::orientation() (handler.rs:206): the EXIF tag of a JPEG, of a WebP through exif_metadata(); none from the PNG decoder; no tag = 1 */
    const int rc = fl::plan_request(src, (uint8_t)(h.orientation ? h.orientation : 1u), query_string, accept_flags, h.input_format, p, plan, result_kind, out_format);
    if (rc) return rc;
    if (*result_kind != FLGPU_RESULT_AS_IS && !h.supported) return FLGPU_ERR_UNSUPPORTED; /* as_is never decodes (handler.rs:202-204) */
    return FLGPU_OK;
}

/* flgpu_process_X_plan (run = false: ctx and dst are not looked at) and flgpu_process_X */
static int process_file(bool run, flgpu_ctx *ctx, SourceKind kind, const uint8_t *file, uint64_t n, const char *query_string, uint32_t accept_flags,
                        flgpu_image *dst, flgpu_plan *plan, int *result_kind, int *out_format)
{
    flgpu_image src;
    flgpu_params p;
    if (!run) return plan_file(kind, file, n, query_string, accept_flags, &src, &p, plan, result_kind, nullptr);
    if (!ctx || !dst) return FLGPU_ERR_INVALID_ARG;
    flgpu_plan local;
    int kind_out = 0;
    const int rc = plan_file(kind, file, n, query_string, accept_flags, &src, &p, plan ? plan : &local, &kind_out, out_format);
    return fl::run_planned(ctx, rc, kind_out, result_kind, &src, &p, dst);
}

/* flgpu_decode_{jpeg,png,webp,webp_lossy}: the file as a source of the identity request -- no dimensions, no operation (and no orientation applied):
   the result is the decoded picture.  (Layout parse only: the CRCs and the streams are read once, in flgpu_transform.) */
static int decode_file(flgpu_ctx *ctx, SourceKind kind, uint32_t src_flags, const uint8_t *file, uint64_t n, flgpu_image *dst)
{
    if (!ctx || !dst || !dst->data || !file) return FLGPU_ERR_INVALID_ARG;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(kind, file, (size_t)n, fl::png_head_opts(src_flags), probe)) return rc;
    if (!probe.head.supported) return FLGPU_ERR_UNSUPPORTED;
    const flgpu_image src = fl::file_image(file, n, probe.head);
    flgpu_params p;
    memset(&p, 0, sizeof(p));
    return flgpu_transform(ctx, &src, &p, dst);
}

extern "C" {

int flgpu_process_jpeg_plan(const uint8_t *jpeg, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_plan *plan, int *result_kind)
try { return process_file(false, nullptr, fl::SRC_JPEG, jpeg, n, query_string, accept_flags, nullptr, plan, result_kind, nullptr); } FL_ABI_CATCH

int flgpu_process_jpeg(flgpu_ctx *ctx, const uint8_t *jpeg, uint64_t n, const char *query_string, uint32_t accept_flags,
                       flgpu_image *dst, flgpu_plan *plan, int *result_kind, int *out_format)
try { return process_file(true, ctx, fl::SRC_JPEG, jpeg, n, query_string, accept_flags, dst, plan, result_kind, out_format); } FL_ABI_CATCH

int flgpu_process_png_plan(const uint8_t *png, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_plan *plan, int *result_kind)
try { return process_file(false, nullptr, fl::SRC_PNG, png, n, query_string, accept_flags, nullptr, plan, result_kind, nullptr); } FL_ABI_CATCH

int flgpu_process_png(flgpu_ctx *ctx, const uint8_t *png, uint64_t n, const char *query_string, uint32_t accept_flags,
                      flgpu_image *dst, flgpu_plan *plan, int *result_kind, int *out_format)
try { return process_file(true, ctx, fl::SRC_PNG, png, n, query_string, accept_flags, dst, plan, result_kind, out_format); } FL_ABI_CATCH

/* (lossless or lossy: file_head goes by the chunk type) */
int flgpu_process_webp_plan(const uint8_t *webp, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_plan *plan, int *result_kind)
try { return process_file(false, nullptr, fl::SRC_WEBP, webp, n, query_string, accept_flags, nullptr, plan, result_kind, nullptr); } FL_ABI_CATCH

int flgpu_process_webp(flgpu_ctx *ctx, const uint8_t *webp, uint64_t n, const char *query_string, uint32_t accept_flags,
                       flgpu_image *dst, flgpu_plan *plan, int *result_kind, int *out_format)
try { return process_file(true, ctx, fl::SRC_WEBP, webp, n, query_string, accept_flags, dst, plan, result_kind, out_format); } FL_ABI_CATCH

int flgpu_decode_jpeg(flgpu_ctx *ctx, const uint8_t *jpeg, uint64_t n, flgpu_image *dst)
try { return decode_file(ctx, fl::SRC_JPEG, 0, jpeg, n, dst); } FL_ABI_CATCH

int flgpu_decode_png_flags(flgpu_ctx *ctx, const uint8_t *png, uint64_t n, uint32_t src_flags, flgpu_image *dst)
try { return decode_file(ctx, fl::SRC_PNG, src_flags, png, n, dst); } FL_ABI_CATCH

int flgpu_decode_png(flgpu_ctx *ctx, const uint8_t *png, uint64_t n, flgpu_image *dst) { return flgpu_decode_png_flags(ctx, png, n, 0, dst); }

int flgpu_decode_webp(flgpu_ctx *ctx, const uint8_t *webp, uint64_t n, flgpu_image *dst)
try { return decode_file(ctx, fl::SRC_WEBP, 0, webp, n, dst); } FL_ABI_CATCH

int flgpu_decode_webp_lossy(flgpu_ctx *ctx, const uint8_t *webp, uint64_t n, flgpu_image *dst)
try { return decode_file(ctx, fl::SRC_VP8, 0, webp, n, dst); } FL_ABI_CATCH

/* ---- what the headers say: the full parse (PNG CRCs, the contents of the WebP streams) ----------------------------------------- */

int flgpu_jpeg_info_of(const uint8_t *jpeg, uint64_t n, flgpu_jpeg_info *info)
try {
    if (!jpeg || !info) return FLGPU_ERR_INVALID_ARG;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(fl::SRC_JPEG, jpeg, (size_t)n, fl::HEAD_FULL, probe)) return rc;
    const fl::JpegInfo &I = probe.jpeg;
    memset(info, 0, sizeof(*info));
    info->width = I.width; info->height = I.height; info->components = I.components;
    info->channels = I.supported ? probe.head.channels : 0u;
    info->adobe_transform = (uint32_t)(I.adobe_transform + 1);
    info->has_icc_profile = I.icc.empty() ? 0u : 1u;
    info->progressive = I.progressive; info->restart_interval = I.restart_interval;
    info->h_max = I.hmax; info->v_max = I.vmax;
    info->exif_orientation = I.exif_orientation; info->supported = I.supported;
    return FLGPU_OK;
} FL_ABI_CATCH

int flgpu_png_info_of_flags(const uint8_t *png, uint64_t n, uint32_t src_flags, flgpu_png_info *info)
try {
    if (!png || !info) return FLGPU_ERR_INVALID_ARG;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(fl::SRC_PNG, png, (size_t)n, fl::HEAD_FULL | ((src_flags & FLGPU_IMG_PNG_ADAM7) ? fl::HEAD_ADAM7 : 0u), probe)) return rc;
    const fl::PngInfo &I = probe.png;
    memset(info, 0, sizeof(*info));
    info->width = I.width; info->height = I.height; info->color_type = I.color_type; info->bit_depth = I.bit_depth;
    info->channels = I.channels; info->interlaced = I.interlaced; info->has_trns = I.has_trns; info->supported = I.supported;
    return FLGPU_OK;
} FL_ABI_CATCH

int flgpu_png_info_of(const uint8_t *png, uint64_t n, flgpu_png_info *info) { return flgpu_png_info_of_flags(png, n, 0, info); }

int flgpu_webp_info_of(const uint8_t *webp, uint64_t n, flgpu_webp_info *info)
try {
    if (!webp || !info) return FLGPU_ERR_INVALID_ARG;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(fl::SRC_WEBP, webp, (size_t)n, fl::HEAD_FULL, probe)) return rc;
    const fl::WebpInfo &I = probe.webp;
    memset(info, 0, sizeof(*info));
    info->width = I.width; info->height = I.height; info->channels = I.channels; info->has_alpha = I.has_alpha;
    info->extended = I.extended; info->animated = I.animated; info->lossless = I.lossless;
    info->exif_orientation = probe.head.orientation;
    info->transforms = I.transforms; info->color_cache_bits = I.color_cache_bits; info->prefix_groups = I.prefix_groups;
    info->supported = I.supported;
    return FLGPU_OK;
} FL_ABI_CATCH

int flgpu_vp8_info_of(const uint8_t *webp, uint64_t n, flgpu_vp8_info *info)
try {
    if (!webp || !info) return FLGPU_ERR_INVALID_ARG;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(fl::SRC_VP8, webp, (size_t)n, fl::HEAD_FULL, probe)) return rc;
    const fl::Vp8Info &I = probe.vp8;
    memset(info, 0, sizeof(*info));
    info->width = I.width; info->height = I.height; info->channels = I.channels; info->has_alpha = I.has_alpha;
    info->extended = I.extended; info->animated = I.animated; info->exif_orientation = probe.head.orientation;
    info->supported = I.supported; info->version = I.version; info->segmentation = I.segmentation; info->update_map = I.update_map;
    info->filter_type = I.filter_simple; info->filter_level = I.filter_level; info->sharpness = I.sharpness; info->partitions = I.partitions;
    info->alpha_compression = I.alpha_compression; info->alpha_filter = I.alpha_filter;
    info->segment_quantizers = I.segment_quantizers; info->segment_filter_levels = I.segment_filter_levels;
    info->coef_prob_updates = I.coef_prob_updates;
    info->macroblocks = I.macroblocks; info->bpred_macroblocks = I.bpred_macroblocks; info->skipped_macroblocks = I.skipped_macroblocks;
    info->skipped_bpred_macroblocks = I.skipped_bpred_macroblocks;
    info->bmodes_mask = I.bmodes_mask; info->ymodes_mask = I.ymodes_mask; info->uvmodes_mask = I.uvmodes_mask;
    info->cat6_tokens = I.cat6_tokens; info->blob_bytes = I.blob_bytes;
    return FLGPU_OK;
} FL_ABI_CATCH

/* ---- the host halves alone.  When *used is written differs, and stays so: the JPEG, PNG and lossless WebP sizes are known from the header and
   written before the capacity check; the lossy WebP and GIF blobs' exact sizes only behind the decode (GIF's first answer is a bound) ------- */

int flgpu_debug_jpeg_blob(const uint8_t *jpeg, uint64_t n, uint8_t *blob, uint64_t capacity, uint64_t *used)
try {
    if (!jpeg || !used) return FLGPU_ERR_INVALID_ARG;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(fl::SRC_JPEG, jpeg, (size_t)n, fl::HEAD_FULL, probe)) return rc;
    if (!probe.head.supported) return FLGPU_ERR_UNSUPPORTED;
    *used = fl::jpeg_blob_bound(probe.jpeg);
    if (!blob) return FLGPU_OK;
    if (capacity < *used) return FLGPU_ERR_BUFFER_TOO_SMALL;
    size_t u = 0;
    const int rc = fl::jpeg_entropy_decode(jpeg, (size_t)n, blob, (size_t)capacity, &u);
    *used = u;
    return rc == 0 ? FLGPU_OK : rc == -2 ? FLGPU_ERR_UNSUPPORTED : FLGPU_ERR_INVALID_ARG;
} FL_ABI_CATCH

int flgpu_debug_png_scanlines_flags(const uint8_t *png, uint64_t n, uint32_t src_flags, uint8_t *out, uint64_t capacity, uint64_t *used)
try {
    if (!png || !used) return FLGPU_ERR_INVALID_ARG;
    const bool adam7 = (src_flags & FLGPU_IMG_PNG_ADAM7) != 0;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(fl::SRC_PNG, png, (size_t)n, fl::HEAD_FULL | (adam7 ? fl::HEAD_ADAM7 : 0u), probe)) return rc;
    if (!probe.head.supported) return FLGPU_ERR_UNSUPPORTED;
    *used = fl::png_scan_bytes(probe.png);
    if (!out) return FLGPU_OK;
    if (capacity < *used) return FLGPU_ERR_BUFFER_TOO_SMALL;
    const int rc = fl::png_decode_scanlines(png, (size_t)n, out, (size_t)capacity, nullptr, adam7);
    return fl::png_status(rc);
} FL_ABI_CATCH

int flgpu_debug_png_scanlines(const uint8_t *png, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used)
{
    return flgpu_debug_png_scanlines_flags(png, n, 0, out, capacity, used);
}

int flgpu_debug_webp_residuals(const uint8_t *webp, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used)
try {
    if (!webp || !used) return FLGPU_ERR_INVALID_ARG;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(fl::SRC_WEBP, webp, (size_t)n, fl::HEAD_FULL, probe)) return rc; // (the blob's size follows from the transform headers)
    if (!probe.head.supported) return FLGPU_ERR_UNSUPPORTED;
    *used = probe.webp.blob_bytes;
    if (!out) return FLGPU_OK;
    if (capacity < probe.webp.blob_bytes) return FLGPU_ERR_BUFFER_TOO_SMALL;
    // the blob in front, the decoder's work area behind it: one buffer, as flgpu_transform has it in its staging
    const size_t cap = fl::webp_blob_capacity(probe.webp, (size_t)n);
    fl::WorkBuf work(cap);
    fl::WebpBlobHeader H;
    const int rc = fl::webp_decode_residuals(webp, (size_t)n, work.p, cap, &H);
    if (rc) return fl::webp_status(rc);
    memcpy(out, work.p, H.total_bytes);
    return FLGPU_OK;
} FL_ABI_CATCH

int flgpu_debug_vp8_blob(const uint8_t *webp, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used)
try {
    if (!webp || !used) return FLGPU_ERR_INVALID_ARG;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(fl::SRC_VP8, webp, (size_t)n, out ? 0u : fl::HEAD_FULL, probe)) return rc; // (the blob's size follows from the tokens)
    if (!probe.head.supported) return FLGPU_ERR_UNSUPPORTED;
    if (!out) { *used = probe.vp8.blob_bytes; return FLGPU_OK; }
    // decoded into a buffer of the worst-case capacity, as flgpu_transform has it in its staging
    const size_t cap = fl::vp8_blob_capacity(probe.vp8);
    fl::WorkBuf work(cap);
    fl::Vp8BlobHeader H;
    const int rc = fl::vp8_decode_levels(webp, (size_t)n, work.p, cap, &H);
    if (rc) return fl::vp8_status(rc);
    *used = H.total_bytes;
    if (capacity < H.total_bytes) return FLGPU_ERR_BUFFER_TOO_SMALL;
    memcpy(out, work.p, H.total_bytes);
    return FLGPU_OK;
} FL_ABI_CATCH

int flgpu_debug_png_inflate_device(flgpu_ctx *ctx, const uint8_t *png, uint64_t n, uint32_t src_flags, uint8_t *out, uint64_t capacity, uint64_t *used)
try {
    if (!ctx || !png || !used) return FLGPU_ERR_INVALID_ARG;
    size_t u = 0;
    const int rc = fl::debug_png_inflate_device(ctx, png, (size_t)n, src_flags, out, (size_t)capacity, &u);
    *used = u;
    return rc;
} FL_ABI_CATCH

int flgpu_debug_png_inflate_model(const uint8_t *png, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used, uint32_t stats[8])
try {
    if (!png || !used) return FLGPU_ERR_INVALID_ARG;
    fl::SourceProbe probe;
    if (int rc = fl::file_head(fl::SRC_PNG, png, (size_t)n, fl::HEAD_FULL | fl::HEAD_ADAM7, probe)) return rc; // (an interlaced stream is the same deflate stream)
    if (!probe.head.supported) return FLGPU_ERR_UNSUPPORTED;
    *used = fl::png_scan_bytes(probe.png);
    if (!out) return FLGPU_OK;
    if (capacity < *used) return FLGPU_ERR_BUFFER_TOO_SMALL;
    const size_t cap = fl::png_stage_bytes(probe.png);
    fl::WorkBuf work(cap);
    fl::PngBlobHeader H;
    if (int rc = fl::png_stage_compressed(png, (size_t)n, work.p, cap, &H, true)) return fl::png_status(rc);
    return fl::png_status(fl::png_inflate_model(work.p, cap, out, (size_t)capacity, stats));
} FL_ABI_CATCH

int flgpu_debug_vp8_planes(flgpu_ctx *ctx, const uint8_t *webp, uint64_t n, int filter, uint8_t *out, uint64_t capacity, uint64_t *used)
try {
    if (!ctx || !webp || !used) return FLGPU_ERR_INVALID_ARG;
    size_t u = 0;
    const int rc = fl::debug_vp8_planes(ctx, webp, (size_t)n, filter, out, (size_t)capacity, &u);
    *used = u;
    return rc;
} FL_ABI_CATCH

/* ---- GIF files: no source of a batch but a batch of their own, so a planner and a runner of their own ---------------------------- */

int flgpu_gif_info_of(const uint8_t *gif, uint64_t n, flgpu_gif_info *info)
try {
    if (!gif || !info) return FLGPU_ERR_INVALID_ARG;
    fl::GifInfo I;
    if (fl::gif_parse_info(gif, (size_t)n, I) != 0) return FLGPU_ERR_PARSE;
    memset(info, 0, sizeof(*info));
    info->width = I.width; info->height = I.height; info->frames = I.frames; info->has_global_table = I.has_global_table;
    info->interlaced_frames = I.interlaced_frames; info->transparent_frames = I.transparent_frames;
    info->disposal_mask = I.disposal_mask; info->max_code_size = I.max_code_size; info->decoded_bytes = I.decoded_bytes;
    info->supported = I.supported;
    if (I.supported) { // whether the file is supported is known only behind the LZW stage (an index beyond its colour table)
        const size_t cap = fl::gif_blob_capacity(I);
        fl::WorkBuf work(cap);
        fl::GifBlobHeader H;
        const int rc = fl::gif_status(fl::gif_decode_blob(gif, (size_t)n, work.p, cap, &H));
        if (rc == FLGPU_ERR_UNSUPPORTED) info->supported = 0;
        else if (rc) return rc;
    }
    return FLGPU_OK;
} FL_ABI_CATCH

static int plan_gif(const uint8_t *gif, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_params *p, flgpu_plan *plan,
                    uint32_t *frames, int *kind, int *out_format)
{
    /* (the container only: flgpu_process_gif runs the LZW stage once; as_is serves the file unread, as the reference does) */
    if (!gif) return FLGPU_ERR_INVALID_ARG;
    fl::GifInfo info;
    if (fl::gif_parse_info(gif, (size_t)n, info) != 0) return FLGPU_ERR_PARSE;
    fl::FileHead canvas_head;
    canvas_head.width = info.width; canvas_head.height = info.height; canvas_head.channels = 4; /* every frame is the Rgba8 canvas (handler.rs:327-333) */
    const flgpu_image canvas = fl::file_image(nullptr, 0, canvas_head);
    if (frames) *frames = info.frames;
    if (!info.supported) return fl::plan_undecodable(query_string, plan, kind, out_format); /* (the canvas may be beyond what a plan can describe) */
    const int rc = fl::plan_request(&canvas, 1, query_string, accept_flags, FLGPU_IN_GIF_FRAME, p, plan, kind, out_format);
    /* FLGPU_ENCODE_GIF: the finished file is what will be attempted (a frame above 256 colours turns it back into pixels, unless
       FLGPU_ENCODE_GIF_QUANTIZE has it quantised -- the plan is the same either way); the per-frame parameters stay as they are,
       one file comes from all the frames */
    if (rc == FLGPU_OK && *kind == FLGPU_RESULT_PIXELS && (accept_flags & FLGPU_ENCODE_GIF) &&
        fl::gif_encodable(plan->out_w, plan->out_h, plan->out_c, info.frames, plan->out_bytes)) {
        *kind = FLGPU_RESULT_GIF_STREAM;
        plan->max_out_bytes = std::max<uint64_t>(plan->out_bytes, fl::gif_max_frame_bytes((uint64_t)plan->out_w * plan->out_h));
    }
    return rc;
}

int flgpu_process_gif_plan(const uint8_t *gif, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_plan *plan, uint32_t *frames,
                           int *result_kind)
try {
    flgpu_params p;
    return plan_gif(gif, n, query_string, accept_flags, &p, plan, frames, result_kind, nullptr);
} FL_ABI_CATCH

int flgpu_process_gif(flgpu_ctx *ctx, const uint8_t *gif, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_image *dst,
                      flgpu_plan *plan, uint32_t *frames, int *result_kind, int *out_format)
try {
    if (!ctx || !dst) return FLGPU_ERR_INVALID_ARG;
    flgpu_params p;
    flgpu_plan local;
    int kind = 0;
    int rc = plan_gif(gif, n, query_string, accept_flags, &p, plan ? plan : &local, frames, &kind, out_format);
    if (result_kind) *result_kind = kind;
    if (rc || kind == FLGPU_RESULT_AS_IS) return rc;
    rc = fl::run_gif_host(ctx, gif, (size_t)n, &p, accept_flags, dst, frames, &kind);
    if (result_kind) *result_kind = kind; /* what happened: the file, or the pixels */
    return rc;
} FL_ABI_CATCH

int flgpu_decode_gif(flgpu_ctx *ctx, const uint8_t *gif, uint64_t n, flgpu_image *dst, uint32_t *frames)
try {
    if (!ctx || !dst || !dst->data || !gif) return FLGPU_ERR_INVALID_ARG;
    return fl::run_gif_host(ctx, gif, (size_t)n, nullptr, 0, dst, frames, nullptr);
} FL_ABI_CATCH

int flgpu_debug_gif_blob(const uint8_t *gif, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used)
try {
    if (!gif || !used) return FLGPU_ERR_INVALID_ARG;
    fl::GifInfo I;
    if (fl::gif_parse_info(gif, (size_t)n, I) != 0) return FLGPU_ERR_PARSE;
    if (!I.supported) return FLGPU_ERR_UNSUPPORTED;
    const size_t cap = fl::gif_blob_capacity(I);
    *used = cap; // (a bound: the palettes the frames share are known only behind the decode)
    if (!out) return FLGPU_OK;
    fl::WorkBuf work(cap);
    fl::GifBlobHeader H;
    const int rc = fl::gif_status(fl::gif_decode_blob(gif, (size_t)n, work.p, cap, &H));
    if (rc) return rc;
    *used = H.total_bytes;
    if (capacity < H.total_bytes) return FLGPU_ERR_BUFFER_TOO_SMALL;
    memcpy(out, work.p, H.total_bytes);
    return FLGPU_OK;
} FL_ABI_CATCH

} // extern "C"
