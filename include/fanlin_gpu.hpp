// fanlin_gpu.hpp -- C++ host-side mirror of the reference's interface for the hot path, over the C ABI of fanlin_gpu.h.
//
// The reference is Rust; a Rust toolchain does not exist where this was built, so the host layer a maintainer would
// write in `src/gpu.rs` is provided here in C++ with the reference's own names, argument meaning
// and error behaviour:
//
//   fanlin::query::Query      src/query.rs:3-94      parse + dimensions / fill_color / quality / cropping / blur /
//                                                    grayscale / inverse / use_avif / use_webp / as_is /
//                                                    unsupported_scale_size
//   fanlin::content::Format   src/content.rs:12-48   accept_webp / webp_accepted / accept_avif / avif_accepted
//   fanlin::handler::State    src/handler.rs:14-52,185-309   new (flgpu_create), process_image (post-decode half)
//
// Errors: the reference returns Result<_, Box<dyn Error>>; here every fallible call throws fanlin::Error carrying the
// flgpu_status and the library's message, which a caller maps onto the same fallback / 500 arm (src/main.rs:185-195).
#ifndef FANLIN_GPU_HPP
#define FANLIN_GPU_HPP

#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "fanlin_gpu.h"

namespace fanlin {

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string &what) : std::runtime_error(what), status(st) {}
};

inline void check(int st, flgpu_ctx *ctx = nullptr)
{
    if (st == FLGPU_OK) return;
    std::string msg = flgpu_strerror(st);
    if (ctx) { const char *d = flgpu_last_error(ctx); if (d && *d) msg += std::string(" (") + d + ")"; }
    throw Error(st, msg);
}

namespace query {
class Query {
public:
    // axum::extract::Query<query::Query>: throws Error{FLGPU_ERR_PARSE} where axum answers 400
    static Query parse(const std::string &query_string) { Query q; check(flgpu_query_parse(query_string.c_str(), &q.raw_)); q.text_ = query_string; return q; }
    std::optional<std::pair<uint32_t, uint32_t>> dimensions() const
    {
        uint32_t w = 0, h = 0;
        if (!flgpu_query_dimensions(&raw_, &w, &h)) return std::nullopt;
        return std::make_pair(w, h);
    }
    std::tuple<uint8_t, uint8_t, uint8_t> fill_color() const { uint8_t r, g, b; flgpu_query_fill_color(&raw_, &r, &g, &b); return {r, g, b}; }
    uint8_t quality() const { return flgpu_query_quality(&raw_); }
    bool cropping() const { return flgpu_query_cropping(&raw_) != 0; }
    float blur() const { return flgpu_query_blur(&raw_); }
    bool grayscale() const { return flgpu_query_grayscale(&raw_) != 0; }
    bool inverse() const { return flgpu_query_inverse(&raw_) != 0; }
    bool use_avif() const { return flgpu_query_use_avif(&raw_) != 0; }
    bool use_webp() const { return flgpu_query_use_webp(&raw_) != 0; }
    bool as_is() const { return flgpu_query_as_is(&raw_) != 0; }
    bool unsupported_scale_size() const { return flgpu_query_unsupported_scale_size(&raw_) != 0; }
    const std::string &text() const { return text_; }
    const flgpu_query &raw() const { return raw_; }

private:
    flgpu_query raw_{};
    std::string text_;
};
} // namespace query

namespace content {
class Format {
public:
    void accept_webp() { flags_ |= FLGPU_ACCEPT_WEBP; }
    bool webp_accepted() const { return (flags_ & FLGPU_ACCEPT_WEBP) == FLGPU_ACCEPT_WEBP; }
    void accept_avif() { flags_ |= FLGPU_ACCEPT_AVIF; }
    bool avif_accepted() const { return (flags_ & FLGPU_ACCEPT_AVIF) == FLGPU_ACCEPT_AVIF; }
    // not a content::Format bit: the library finishes image/png bodies for PNG inputs that stay PNG (FLGPU_RESULT_PNG_STREAM)
    void encode_png() { flags_ |= FLGPU_ENCODE_PNG; }
    // not a content::Format bit: process_png also takes Adam7-interlaced files of up to 8 bits per sample
    void decode_png_adam7() { flags_ |= FLGPU_DECODE_PNG_ADAM7; }
    // not a content::Format bit: process_png has the file's deflate stream inflated on the device (FLGPU_IMG_PNG_INFLATE)
    void decode_png_inflate() { flags_ |= FLGPU_DECODE_PNG_INFLATE; }
    // not a content::Format bit: the library finishes lossless image/webp bodies, the WebP arm at quality 100
    // (FLGPU_RESULT_WEBP_STREAM)
    void encode_webp_lossless() { flags_ |= FLGPU_ENCODE_WEBP_LOSSLESS; }
    // not a content::Format bit: process_gif finishes the image/gif body where no frame has more than 256 colours
    // (FLGPU_RESULT_GIF_STREAM)
    void encode_gif() { flags_ |= FLGPU_ENCODE_GIF; }
    // ... and also where a frame has more: such a frame is quantised on the device to at most 256 entries (the library's own rule)
    void encode_gif_quantize() { flags_ |= FLGPU_ENCODE_GIF | FLGPU_ENCODE_GIF_QUANTIZE; }
    // not a content::Format bit: the library finishes lossy image/webp bodies, the WebP arm below quality 100
    // (FLGPU_RESULT_WEBP_STREAM; outputs over FLGPU_FE_WEBP_LOSSY's limits still come back as planes)
    void encode_webp_lossy() { flags_ |= FLGPU_ENCODE_WEBP_LOSSY; }
    // ... and from FLGPU_FE_WEBP_LOSSY_I4 (macroblocks may be B_PRED: smaller files, a slower analysis) where the output fits it
    void encode_webp_lossy_i4() { flags_ |= FLGPU_ENCODE_WEBP_LOSSY | FLGPU_ENCODE_WEBP_LOSSY_I4; }
    // ... with per-picture coefficient probabilities (FLGPU_FE_WEBP_LOSSY_AP, or FLGPU_FE_WEBP_LOSSY_I4_AP after encode_webp_lossy_i4():
    // the same pictures in fewer bytes)
    void encode_webp_lossy_probs() { flags_ |= FLGPU_ENCODE_WEBP_LOSSY | FLGPU_ENCODE_WEBP_LOSSY_PROBS; }
    // ... with a loop filter level picked on the device: the _LF twin of whichever front end the calls above select
    void encode_webp_lossy_filter() { flags_ |= FLGPU_ENCODE_WEBP_LOSSY | FLGPU_ENCODE_WEBP_LOSSY_FILTER; }
    // ... with the alpha plane of a translucent picture as a VP8L stream wherever that is smaller: FLGPU_FEO_ALPHA_VP8L on
    // whichever front end the calls above select
    void encode_webp_lossy_alpha() { flags_ |= FLGPU_ENCODE_WEBP_LOSSY | FLGPU_ENCODE_WEBP_LOSSY_ALPHA; }
    // ... with segment-adaptive quantisers (up to four classes of macroblocks by activity): FLGPU_FEO_SEGMENTS on whichever front
    // end the calls above select
    void encode_webp_lossy_segments() { flags_ |= FLGPU_ENCODE_WEBP_LOSSY | FLGPU_ENCODE_WEBP_LOSSY_SEGMENTS; }
    // a JPEG that stays JPEG is coded with Huffman tables from the picture's own symbol counts (FLGPU_FEO_JPEG_OPTIMIZE): the same
    // pixels in a smaller file, today's file where the tables do not pay
    void encode_jpeg_optimize() { flags_ |= FLGPU_ENCODE_JPEG_OPTIMIZE; }
    // a JPEG that stays JPEG is coded with 4:2:0 chroma subsampling (FLGPU_FEO_JPEG_420): smaller files, other pixels; alone or with the above
    void encode_jpeg_420() { flags_ |= FLGPU_ENCODE_JPEG_420; }
    // a JPEG that stays JPEG is written as a progressive file of five scans (FLGPU_FEO_JPEG_PROGRESSIVE): the baseline file's pixels, the whole picture
    // after the first few hundred bytes; the same file with encode_jpeg_optimize(), ignored beside encode_jpeg_420()
    void encode_jpeg_progressive() { flags_ |= FLGPU_ENCODE_JPEG_PROGRESSIVE; }
    uint32_t flags() const { return flags_; }

private:
    uint32_t flags_ = 0;
};
} // namespace content

namespace handler {

// DynamicImage as the decoder leaves it: tightly packed rows, 1 = Luma8, 2 = LumaA8, 3 = Rgb8, 4 = Rgba8
struct Decoded {
    const uint8_t *pixels;
    uint32_t width, height, channels;
    uint8_t orientation = 1;                        // decoder.orientation() as an EXIF code
    flgpu_input_format format = FLGPU_IN_JPEG;      // what with_guessed_format() said
};

struct Processed {
    flgpu_result_kind kind;        // AS_IS: serve the original bytes; JPEG_STREAM / PNG_STREAM / WEBP_STREAM: body is final; WEBP_PLANES / PIXELS: host encoder
    flgpu_out_format negotiated;   // container chosen at src/handler.rs:256-261
    flgpu_plan plan;               // geometry of what `data` holds
    uint32_t flags;                // FLGPU_IMG_*
    std::vector<uint8_t> data;
};

class State {
public:
    // handler::State::new: one context per process, shared by all workers (internally synchronised)
    explicit State(int device = -1, uint32_t max_batch = 0, uint32_t flush_timeout_us = 0, uint32_t queue_lanes = 0)
    {
        flgpu_config cfg{};
        cfg.device = device; cfg.max_batch = max_batch; cfg.flush_timeout_us = flush_timeout_us; cfg.queue_lanes = queue_lanes;
        int st = 0;
        ctx_ = flgpu_create(&cfg, &st);
        if (!ctx_) check(st ? st : FLGPU_ERR_NO_DEVICE);
    }
    ~State() { if (ctx_) flgpu_destroy(ctx_); }
    State(const State &) = delete;
    State &operator=(const State &) = delete;

    // create_cmyk_to_rgb_converter (src/main.rs:74-76)
    void set_cmyk_profile(const std::vector<uint8_t> &icc) { check(flgpu_set_cmyk_profile(ctx_, icc.data(), icc.size()), ctx_); }

    // convert_jpeg_color_if_needed's colour half (src/handler.rs:421-466): n x 4 bytes in, n x 3 out
    std::vector<uint8_t> cmyk_to_rgb(const std::vector<uint8_t> &cmyk, bool ycck, const std::vector<uint8_t> *embedded_icc = nullptr)
    {
        std::vector<uint8_t> rgb(cmyk.size() / 4 * 3);
        check(flgpu_cmyk_to_rgb(ctx_, cmyk.data(), cmyk.size() / 4, rgb.data(), embedded_icc ? embedded_icc->data() : nullptr,
                                embedded_icc ? embedded_icc->size() : 0, ycck ? FLGPU_CMYK_INPUT_YCCK : 0u), ctx_);
        return rgb;
    }

    // State::process_image after the decoder (src/handler.rs:198-308): blocking, safe to call from many threads at once
    Processed process_image(const Decoded &img, const query::Query &params, const content::Format &content)
    {
        const flgpu_image src{const_cast<uint8_t *>(img.pixels), (uint64_t)img.width * img.height * img.channels, img.width, img.height, img.channels, 0, 0};
        const char *q = params.text().c_str();
        return process(
            [&](flgpu_plan *plan, int *kind) { return flgpu_process_image_plan(&src, img.orientation, q, content.flags(), img.format, plan, kind); },
            // a PNG or lossless WebP body is staged at the format's worst case, so that it never comes back too small
            [](const Processed &o) { return o.kind == FLGPU_RESULT_PNG_STREAM || o.kind == FLGPU_RESULT_WEBP_STREAM ? o.plan.max_out_bytes : o.plan.out_bytes; },
            [&](flgpu_image *dst, flgpu_plan *plan, int *kind, int *fmt) { return flgpu_process_image(ctx_, &src, img.orientation, q, content.flags(), img.format, dst, plan, kind, fmt); });
    }

    // PngDecoder::new's view of a file (src/handler.rs:218-220): false if the bytes are no intact PNG container
    static bool png_info(const std::vector<uint8_t> &file, flgpu_png_info &info) { return flgpu_png_info_of(file.data(), file.size(), &info) == FLGPU_OK; }

    // State::process_image for a PNG input from the file bytes on: inflate on this thread, row filters, expansion, pixel pipeline and
    // (with FLGPU_ENCODE_PNG in the content flags) the PNG encoder on the device.  Throws on files the decoder does not cover
    // (FLGPU_ERR_UNSUPPORTED: 16-bit samples, Adam7) and on damaged ones (FLGPU_ERR_PARSE): the host then uses its own decoder.
    Processed process_png(const std::vector<uint8_t> &file, const query::Query &params, const content::Format &content)
    {
        return process_file(flgpu_process_png_plan, flgpu_process_png, file, params, content);
    }

    // WebPDecoder::new's view of a file (src/handler.rs:205-220): false if the bytes are no intact WebP container
    static bool webp_info(const std::vector<uint8_t> &file, flgpu_webp_info &info) { return flgpu_webp_info_of(file.data(), file.size(), &info) == FLGPU_OK; }

    // the same for a lossy WebP file (`VP8 `, with or without VP8X / ALPH): false if the bytes are no intact lossy WebP file
    static bool vp8_info(const std::vector<uint8_t> &file, flgpu_vp8_info &info) { return flgpu_vp8_info_of(file.data(), file.size(), &info) == FLGPU_OK; }

    // libwebp's WebPDecodeRGB / WebPDecodeRGBA of a lossy WebP file on the device: width x height x info.channels bytes, no orientation applied
    std::vector<uint8_t> decode_webp_lossy(const std::vector<uint8_t> &file)
    {
        flgpu_vp8_info info;
        check(flgpu_vp8_info_of(file.data(), file.size(), &info));
        std::vector<uint8_t> px((size_t)info.width * info.height * (info.channels ? info.channels : 1u));
        flgpu_image dst{px.data(), px.size(), 0, 0, 0, 0, 0};
        check(flgpu_decode_webp_lossy(ctx_, file.data(), file.size(), &dst), ctx_);
        return px;
    }

    // State::process_image for a WebP input from the file bytes on (lossless, or lossy: the library goes by the chunk type), with the
    // file's EXIF orientation: entropy decode on this
    // thread, inverse transforms, pixel pipeline and (with FLGPU_ENCODE_WEBP_LOSSLESS in the content flags, quality=100) the lossless
    // WebP encoder on the device.  Throws on files the decoders do not cover (FLGPU_ERR_UNSUPPORTED: animated files, the refused frame-header
    // features of a lossy one) and on damaged
    // ones (FLGPU_ERR_PARSE): the host then uses its own decoder.
    Processed process_webp(const std::vector<uint8_t> &file, const query::Query &params, const content::Format &content)
    {
        return process_file(flgpu_process_webp_plan, flgpu_process_webp, file, params, content);
    }

    // GifDecoder::new's view of a file (src/handler.rs:311-321), LZW stage included: false if the file is damaged
    static bool gif_info(const std::vector<uint8_t> &file, flgpu_gif_info &info) { return flgpu_gif_info_of(file.data(), file.size(), &info) == FLGPU_OK; }

    // process_gif from the file bytes on (src/handler.rs:311-353): LZW on this thread, compositing and the per-frame pipeline on the
    // device.  `data` holds `frames` results plan.out_bytes apart, for the GIF encoder (handler.rs:355-363); with encode_gif() in
    // `accepted` and no frame above 256 colours it holds the finished file instead (kind FLGPU_RESULT_GIF_STREAM; handler.rs:355-364
    // on the device too).  Throws on files the decoder does not vouch for (FLGPU_ERR_UNSUPPORTED) and on damaged ones
    // (FLGPU_ERR_PARSE): the host then decodes the frames itself and hands them to flgpu_transform_batch.
    Processed process_gif(const std::vector<uint8_t> &file, const query::Query &params, uint32_t &frames, const content::Format &accepted = content::Format())
    {
        const char *q = params.text().c_str();
        return process(
            [&](flgpu_plan *plan, int *kind) { return flgpu_process_gif_plan(file.data(), file.size(), q, accepted.flags(), plan, &frames, kind); },
            // (a planned stream may still come back as pixels: 64 + frames x max_out_bytes holds either)
            [&](const Processed &o) { return o.kind == FLGPU_RESULT_GIF_STREAM ? 64 + o.plan.max_out_bytes * frames : o.plan.out_bytes * frames; },
            [&](flgpu_image *dst, flgpu_plan *plan, int *kind, int *fmt) { return flgpu_process_gif(ctx_, file.data(), file.size(), q, accepted.flags(), dst, plan, &frames, kind, fmt); });
    }

    flgpu_ctx *raw() { return ctx_; }

private:
    // What the four process_* calls share: plan, size, run, shrink.  plan(plan, kind) and run(dst, plan, kind, fmt) are one format's two ABI calls,
    // bytes(out) is what to reserve for the planned result.
    template <class Plan, class Bytes, class Run>
    Processed process(Plan plan, Bytes bytes, Run run)
    {
        Processed out{};
        int kind = 0, fmt = FLGPU_OUT_KEEP;
        check(plan(&out.plan, &kind));
        out.kind = static_cast<flgpu_result_kind>(kind);
        out.negotiated = FLGPU_OUT_KEEP;
        if (out.kind == FLGPU_RESULT_AS_IS) return out;
        out.data.resize(bytes(out));
        flgpu_image dst{out.data.data(), out.data.size(), 0, 0, 0, 0, 0};
        check(run(&dst, &out.plan, &kind, &fmt), ctx_);
        out.kind = static_cast<flgpu_result_kind>(kind); // what happened: a GIF planned as a stream may come back as pixels (the others report the planned kind again)
        out.negotiated = static_cast<flgpu_out_format>(fmt);
        out.flags = dst.flags;
        out.data.resize(dst.bytes);
        return out;
    }

    // process_png / process_webp: a file staged at its format's worst case (max_out_bytes)
    template <class PlanFn, class RunFn>
    Processed process_file(PlanFn plan_fn, RunFn run_fn, const std::vector<uint8_t> &file, const query::Query &params, const content::Format &content)
    {
        const char *q = params.text().c_str();
        return process(
            [&](flgpu_plan *plan, int *kind) { return plan_fn(file.data(), file.size(), q, content.flags(), plan, kind); },
            [](const Processed &o) { return o.plan.max_out_bytes; },
            [&](flgpu_image *dst, flgpu_plan *plan, int *kind, int *fmt) { return run_fn(ctx_, file.data(), file.size(), q, content.flags(), dst, plan, kind, fmt); });
    }

    flgpu_ctx *ctx_ = nullptr;
};

} // namespace handler
} // namespace fanlin

#endif
