// fl_gifrun.cpp -- a GIF file from bytes to results: the LZW stage on the calling thread (fl_gifsrc.cpp), the compose kernel, the frames as one
// device batch through run_batch_device, and -- FLGPU_ENCODE_GIF -- the encoder behind it.  A caller of the batch runner, not part of it.
#include <algorithm>

#include "fl_context.h"

namespace fl {

// The compose phase: `blob` is the DEVICE copy of what gif_decode_blob left, H its header.  Runs gif_compose_kernel into scratch
// and describes the H.frames composited canvases as device-resident Rgba8 sources in dsrc[0 .. H.frames).
static int decode_gif_sources(flgpu_ctx *c, const GifBlobHeader &H, const uint8_t *blob, flgpu_image *dsrc, hipStream_t st)
{
    const size_t plane = (size_t)H.width * H.height * 4u;
    FL_HIP(c, c->d_gifdec.reserve((size_t)H.frames * plane + 256), "GIF decode scratch");
    uint8_t *frames = static_cast<uint8_t *>(c->d_gifdec.p);
    { ProfileScope ps(c, st, 5); FL_HIP(c, launch_gif_compose(blob, H.width, H.height, H.frames, frames, st), "GIF compose kernel"); }
    for (uint32_t f = 0; f < H.frames; ++f) {
        memset(&dsrc[f], 0, sizeof(dsrc[f]));
        dsrc[f].data = frames + (size_t)f * plane;
        dsrc[f].capacity = plane;
        dsrc[f].width = H.width; dsrc[f].height = H.height; dsrc[f].channels = 4;
    }
    c->gif_sources++; c->gif_frames += H.frames; c->gif_upload_bytes += H.total_bytes;
    return FLGPU_OK;
}

// The encode phase behind run_batch_device: the frames lie in d_out at `pitch`; the six kernels of fl_gif.hip leave the file and
// its status record in scratch.  Enqueues only.
// `quantize` (FLGPU_ENCODE_GIF_QUANTIZE): frames above 256 colours get a table from fl_gifquant.hip, whose cells are planned here too.
static int encode_gif_frames(flgpu_ctx *c, const flgpu_plan &plan, uint32_t frames, size_t pitch, uint64_t frame_max, bool quantize, const uint8_t **file, hipStream_t st)
{
    GifEncJob J;
    memset(&J, 0, sizeof(J));
    J.w = plan.out_w; J.h = plan.out_h; J.c = plan.out_c; J.frames = frames;
    J.px = plan.out_w * plan.out_h; J.nseg = (uint32_t)gif_segments(J.px);
    J.pixels = static_cast<const uint8_t *>(c->d_out.p); J.pix_pitch = pitch;
    J.idx_pitch = align_up((size_t)J.px, 16) + 16; J.body_pitch = align_up((size_t)frame_max, 16);
    J.quant = quantize && gif_quantizable(J.px, frames) ? 1u : 0u; // (else a frame above 256 colours sends the file back as pixels, as without the bit)
    J.qstride = gif_quant_stride(J.px);
    const size_t segs = (size_t)frames * J.nseg;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += align_up(bytes, 256); return at; };
    const size_t o_status = carve(16), o_frec = carve((size_t)frames * kGifFrameRec * 4), o_ckeys = carve((size_t)frames * kGifColourSlots * 4),
                 o_cvals = carve((size_t)frames * kGifColourSlots * 4), o_idx = carve((size_t)frames * J.idx_pitch),
                 o_segs = carve(segs * kGifSegDwords * 4), o_bits = carve(segs * 4), o_off = carve(segs * 4),
                 o_bodies = carve((size_t)frames * J.body_pitch), o_file = carve((size_t)gif_max_file_bytes(frames, frame_max)),
                 o_qcells = carve(J.quant ? (size_t)frames * 4u * J.qstride * 4 : 0), o_qbox = carve(J.quant ? (size_t)frames * J.qstride * 4 : 0);
    FL_HIP(c, c->d_gifenc.reserve(off), "GIF encode scratch");
    FL_HIP(c, c->h_gifstat.reserve(16), "pinned GIF encode status");
    uint8_t *base = static_cast<uint8_t *>(c->d_gifenc.p);
    J.status = reinterpret_cast<uint32_t *>(base + o_status); J.frec = reinterpret_cast<uint32_t *>(base + o_frec);
    J.ckeys = reinterpret_cast<uint32_t *>(base + o_ckeys); J.cvals = reinterpret_cast<uint32_t *>(base + o_cvals);
    J.indices = base + o_idx; J.segs = reinterpret_cast<uint32_t *>(base + o_segs);
    J.seg_bits = reinterpret_cast<uint32_t *>(base + o_bits); J.seg_off = reinterpret_cast<uint32_t *>(base + o_off);
    J.bodies = base + o_bodies; J.file = base + o_file;
    if (J.quant) { J.qcells = reinterpret_cast<uint32_t *>(base + o_qcells); J.qbox = reinterpret_cast<uint32_t *>(base + o_qbox); }
    *file = J.file;
    FL_HIP(c, hipMemsetAsync(J.status, 0, 16, st), "GIF encode status");
    { ProfileScope ps(c, st, 6); FL_HIP(c, launch_gif_encode(J, st), "GIF encode kernels"); }
    FL_HIP(c, hipMemcpyAsync(c->h_gifstat.p, J.status, 16, hipMemcpyDeviceToHost, st), "GIF encode status D2H");
    return FLGPU_OK;
}

int run_gif_host(flgpu_ctx *c, const uint8_t *gif, size_t n, const flgpu_params *params, uint32_t accept_flags, flgpu_image *dst, uint32_t *frames, int *result_kind)
{
    if (!gif || !dst || !dst->data) return FLGPU_ERR_INVALID_ARG;
    // the serial half on the calling thread, before any device work and outside the context's lock: callers decode side by side
    GifInfo info;
    if (gif_parse_info(gif, n, info) != 0) { c->set_error("malformed GIF file (signature, logical screen, block layout, colour table or too few bytes)"); return FLGPU_ERR_PARSE; }
    if (!info.supported) { c->set_error("GIF file not covered by the device decoder (no frames, a frame outside the canvas or without area, code size, frame count, decoded size)"); return FLGPU_ERR_UNSUPPORTED; }
    flgpu_plan plan;
    memset(&plan, 0, sizeof(plan));
    const size_t canvas = (size_t)info.width * info.height * 4u;
    if (params) {
        if (fe_encoded(params->front_end)) return FLGPU_ERR_INVALID_ARG; // (GIF encode is not a per-picture front end: one file comes from all the frames, FLGPU_ENCODE_GIF below)
        if (int rc = flgpu_plan_output(params, info.width, info.height, 4, &plan)) return rc;
    }
    const size_t each = params ? (size_t)plan.out_bytes : canvas;
    // FLGPU_ENCODE_GIF: the file is attempted; the destination holds either outcome
    const bool encode = params && (accept_flags & FLGPU_ENCODE_GIF) && gif_encodable(plan.out_w, plan.out_h, plan.out_c, info.frames, plan.out_bytes);
    const bool quantize = encode && (accept_flags & FLGPU_ENCODE_GIF_QUANTIZE);
    const uint64_t frame_max = encode ? gif_max_frame_bytes((uint64_t)plan.out_w * plan.out_h) : 0;
    if (result_kind) *result_kind = FLGPU_RESULT_PIXELS;
    if (encode && dst->capacity < gif_max_file_bytes(info.frames, std::max<uint64_t>(frame_max, plan.out_bytes))) return FLGPU_ERR_BUFFER_TOO_SMALL;
    if (dst->capacity < (uint64_t)each * info.frames) return FLGPU_ERR_BUFFER_TOO_SMALL;
    std::vector<uint8_t> blob(gif_blob_capacity(info));
    GifBlobHeader H;
    const int drc = gif_decode_blob(gif, n, blob.data(), blob.size(), &H);
    if (drc == kGifParse) c->set_error("malformed GIF stream (an LZW code beyond the table, or fewer indices than the frame has pixels)");
    if (drc == kGifUnsupported) c->set_error("GIF frame with an index beyond its colour table");
    if (drc) return gif_status(drc);

    flgpu_ctx *s = c->shard_ctx.empty() ? c : c->shard_ctx[0]; // one file, one device
    std::lock_guard<std::mutex> g(s->mu);
    FL_HIP(s, hipSetDevice(s->device), "hipSetDevice");
    hipStream_t st = s->stream;
    if (s->last_stream && s->last_stream != st && s->last_done) FL_HIP(s, hipStreamWaitEvent(st, s->last_done, 0), "stream handoff");
    FL_HIP(s, s->d_in.reserve(H.total_bytes), "device input staging");
    FL_HIP(s, s->h_stage_in.reserve(H.total_bytes), "pinned input staging");
    memcpy(s->h_stage_in.p, blob.data(), H.total_bytes);
    FL_HIP(s, hipMemcpyAsync(s->d_in.p, s->h_stage_in.p, H.total_bytes, hipMemcpyHostToDevice, st), "H2D");
    std::vector<flgpu_image> dsrc(H.frames);
    if (int rc = decode_gif_sources(s, H, static_cast<const uint8_t *>(s->d_in.p), dsrc.data(), st)) return rc;
    s->gif_file_bytes += n;
    if (frames) *frames = H.frames;
    dst->width = info.width; dst->height = info.height; dst->channels = 4; dst->flags = 0;
    if (!params) { // the composited frames themselves
        FL_HIP(s, hipMemcpyAsync(dst->data, s->d_gifdec.p, canvas * H.frames, hipMemcpyDeviceToHost, st), "D2H");
        FL_HIP(s, hipStreamSynchronize(st), "GIF decode sync");
        dst->bytes = (uint64_t)canvas * H.frames;
        return FLGPU_OK;
    }
    // the per-frame pipeline: every frame the same request, one device batch
    const size_t pitch = align_up(plan.max_out_bytes, 256);
    FL_HIP(s, s->d_out.reserve(pitch * H.frames), "device output staging");
    FL_HIP(s, s->h_stage_out.reserve(std::max<size_t>(pitch * H.frames, encode ? (size_t)gif_max_file_bytes(H.frames, frame_max) : 0)), "pinned output staging");
    std::vector<flgpu_image> ddst(H.frames);
    for (uint32_t f = 0; f < H.frames; ++f) {
        memset(&ddst[f], 0, sizeof(ddst[f]));
        ddst[f].data = static_cast<uint8_t *>(s->d_out.p) + pitch * f;
        ddst[f].capacity = plan.max_out_bytes;
    }
    int rc = run_batch_device(s, H.frames, dsrc.data(), params, true, ddst.data(), st);
    if (rc) return rc;
    // the frames as pixels: out of the pitched staging (its D2H has completed), `each` bytes apart
    auto frames_out = [&] {
        for (uint32_t f = 0; f < H.frames; ++f) memcpy(dst->data + each * f, static_cast<const uint8_t *>(s->h_stage_out.p) + pitch * f, each);
        dst->width = plan.out_w; dst->height = plan.out_h; dst->channels = plan.out_c; dst->flags = ddst[0].flags;
        dst->bytes = (uint64_t)each * H.frames;
        return FLGPU_OK;
    };
    if (encode) {
        // the device decides: one small status record comes back, then the file or -- a frame above 256 colours that is not
        // quantised -- the pixels
        const uint8_t *file = nullptr;
        rc = encode_gif_frames(s, plan, H.frames, pitch, frame_max, quantize, &file, st);
        if (rc) return rc;
        rc = collect_results(s, H.frames, ddst.data(), st);
        if (rc) return rc;
        const uint32_t *status = static_cast<const uint32_t *>(s->h_gifstat.p);
        if (!status[0]) {
            const uint64_t bytes = status[1];
            if (bytes <= kGifFileHead || bytes > gif_max_file_bytes(H.frames, frame_max)) { s->set_error("GIF encode: file length outside its bounds"); return FLGPU_ERR_DEVICE; }
            FL_HIP(s, hipMemcpyAsync(s->h_stage_out.p, file, bytes, hipMemcpyDeviceToHost, st), "D2H");
            FL_HIP(s, hipStreamSynchronize(st), "GIF encode sync");
            memcpy(dst->data, s->h_stage_out.p, bytes);
            dst->width = plan.out_w; dst->height = plan.out_h; dst->channels = plan.out_c; dst->flags = FLGPU_IMG_ENCODED;
            dst->bytes = bytes;
            s->gif_encoded++; s->gif_encoded_bytes += bytes; s->gif_quantized_frames += status[2];
            if (result_kind) *result_kind = FLGPU_RESULT_GIF_STREAM;
            return FLGPU_OK;
        }
        s->gif_encode_fallbacks++;
        FL_HIP(s, hipMemcpyAsync(s->h_stage_out.p, s->d_out.p, pitch * H.frames, hipMemcpyDeviceToHost, st), "D2H");
        FL_HIP(s, hipStreamSynchronize(st), "GIF frames sync");
        return frames_out();
    }
    FL_HIP(s, hipMemcpyAsync(s->h_stage_out.p, s->d_out.p, pitch * H.frames, hipMemcpyDeviceToHost, st), "D2H");
    rc = collect_results(s, H.frames, ddst.data(), st);
    if (rc) return rc;
    return frames_out();
}

} // namespace fl
