/*
 * fanlin_gpu.h -- C ABI of the MI355X-native image hot path for fanlin-rs.
 *
 * This is the drop-in boundary: a reference-side shim (Rust `extern "C"`
 * block) binds exactly these entry points and keeps the
 * rest of fanlin-rs (axum handler, routing, origin fetch, codecs' entropy
 * stages) unchanged.  Plain pointers and sizes only; no C++ or torch types;
 * no exceptions cross this boundary; every function returns an flgpu_status
 * (0 = ok) unless it returns a pointer.
 *
 * What each entry point replaces in the reference (paths relative to the
 * fanlin-rs repository root):
 *
 *   flgpu_query_parse / flgpu_query_*   src/query.rs:3-94   (query::Query + accessors)
 *   FLGPU_ACCEPT_* flags                src/content.rs:12-48 (content::Format)
 *   flgpu_params_from_query             src/handler.rs:224-261 (which accessors feed which step)
 *   flgpu_plan_output                   image::math::utils::resize_dimensions +
 *                                       DynamicImage::resize / resize_to_fill geometry +
 *                                       the letterbox rule at src/handler.rs:229-249
 *   flgpu_transform*                    img.apply_orientation (src/handler.rs:221-223) and the image-crate calls at
 *                                       src/handler.rs:225,227,233,
 *                                       235,240-247,253 (grayscale, invert, resize,
 *                                       resize_to_fill, from_pixel + overlay, blur)
 *   front_end = FLGPU_FE_JFIF444        colour front end of jpeg::JpegEncoder::encode_image,
 *                                       src/handler.rs:274-278
 *   front_end = FLGPU_FE_WEBP420        WebPPictureImportRGBA + ARGB->YUV420 inside
 *                                       webp::Encoder::encode, src/handler.rs:295-297
 *   front_end = FLGPU_FE_JPEG           the whole jpeg::JpegEncoder::new_with_quality(q).encode_image(&img),
 *                                       src/handler.rs:274-278 (FDCT, quantiser, Huffman coder, framing)
 *   front_end = FLGPU_FE_PNG            the whole PngEncoder::new_with_quality(ct, FilterType::Adaptive) +
 *                                       img.write_with_encoder, src/handler.rs:264-273 (row filters, deflate, framing)
 *   front_end = FLGPU_FE_WEBP_LOSSLESS  image's lossless WebP encoder for q == 100 after img.into_rgba8(),
 *                                       src/handler.rs:286-292 (transforms, prefix codes, runs, framing)
 *   front_end = FLGPU_FE_WEBP_LOSSY     webp::Encoder::from_image(&img).encode(q) for q < 100, src/handler.rs:293-297
 *                                       (a VP8 key-frame coder of this library's own choices, not libwebp's)
 *   params.filter = NEAREST             the per-frame pipeline of process_gif, src/handler.rs:327-353
 *   flgpu_process_image                 State::process_image after the decoder as one call, src/handler.rs:198-308
 *   flgpu_ycck_to_cmyk                  the YCCK loop of convert_jpeg_color_if_needed, src/handler.rs:423-438
 *   flgpu_set_cmyk_profile / _clut      create_cmyk_to_rgb_converter + CMYK2RGB::with_icc_profile,
 *                                       src/main.rs:74-76, src/handler.rs:469-488
 *   flgpu_cmyk_to_rgb[_device]          CMYK2RGB::convert = lcms2 transform_pixels, src/handler.rs:446-462,490-492
 *   FLGPU_IMG_JPEG_SOURCE / flgpu_process_jpeg   JpegDecoder::new + DynamicImage::from_decoder, src/handler.rs:205-220
 *   FLGPU_IMG_PNG_SOURCE / flgpu_process_png     PngDecoder + DynamicImage::from_decoder, src/handler.rs:218-220
 *   FLGPU_IMG_WEBP_SOURCE / flgpu_process_webp   WebPDecoder (lossless VP8L) + DynamicImage::from_decoder and its EXIF orientation,
 *                                                src/handler.rs:205-220
 *   flgpu_process_gif / flgpu_decode_gif         GifDecoder::new + into_frames().collect_frames() and the per-frame pipeline of
 *                                                process_gif, src/handler.rs:311-353
 *   flgpu_create / flgpu_destroy        lifetime of handler::State, src/handler.rs:14-21,36-52
 *   flgpu_config.devices / flgpu_plan_shards   the one shared Arc<State> behind all tokio workers, src/main.rs:108-112
 */
#ifndef FANLIN_GPU_H
#define FANLIN_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLGPU_ABI_VERSION 6

typedef enum flgpu_status {
    FLGPU_OK = 0,
    FLGPU_ERR_INVALID_ARG = 1,   /* null pointer, zero-sized image, channels not in 1..4, ... */
    FLGPU_ERR_UNSUPPORTED = 2,   /* valid request the device path does not cover */
    FLGPU_ERR_NO_DEVICE = 3,     /* no usable HIP device: the library never falls back to the CPU */
    FLGPU_ERR_OOM = 4,           /* host or device allocation failed */
    FLGPU_ERR_DEVICE = 5,        /* a HIP call failed; see flgpu_last_error() */
    FLGPU_ERR_PARSE = 6,         /* query string rejected (axum would answer 400); a PNG, WebP or GIF source that is damaged */
    FLGPU_ERR_BUFFER_TOO_SMALL = 7,
    FLGPU_ERR_SHUTDOWN = 8       /* context is being destroyed */
} flgpu_status;

/* Decoded image as the image crate holds it: tightly packed rows, top-left
 * origin, interleaved u8 channels; 1 = Luma8, 2 = LumaA8, 3 = Rgb8, 4 = Rgba8. */
typedef struct flgpu_image {
    uint8_t *data;      /* host pointer (flgpu_transform, _batch) or device pointer (_batch_device) */
    uint64_t capacity;  /* src: bytes valid at data; dst: bytes writable at data */
    uint32_t width, height, channels;
    uint32_t flags;     /* out: FLGPU_IMG_* */
    uint64_t bytes;     /* out: bytes produced at data (pixels, planes or an encoded stream) */
} flgpu_image;

#define FLGPU_IMG_FRONTEND_PLANES 1u  /* dst->data holds encoder planes, not interleaved pixels */
#define FLGPU_IMG_PINNED          8u  /* in (src and dst of flgpu_transform): data comes from flgpu_host_alloc, i.e. is page-locked:
                                         the copy through the library's own pinned staging blocks is skipped */
#define FLGPU_IMG_ENCODED         4u  /* JPEG: data holds an encoded stream of `bytes` bytes */
#define FLGPU_IMG_JPEG_SOURCE     16u /* in (src of flgpu_transform / flgpu_transform_batch): data holds a baseline JPEG FILE of `capacity`
                                         bytes instead of pixels, width / height / channels say what it decodes to (flgpu_jpeg_info):
                                         the library decodes it itself -- Huffman decoding on the calling thread, dequantisation, IDCT,
                                         chroma up-sampling and YCbCr -> RGB on the device -- replacing JpegDecoder::new +
                                         DynamicImage::from_decoder (src/handler.rs:205-220).  ~1 MB crosses PCIe instead of 6.2 MB
                                         for a 1080p picture.  Streams it does not cover: FLGPU_ERR_UNSUPPORTED (decode on the host). */
#define FLGPU_IMG_PNG_SOURCE      32u /* in (src of flgpu_transform / flgpu_transform_batch): data holds a PNG FILE of `capacity` bytes instead of
                                         pixels, width / height / channels say what it decodes to (flgpu_png_info_of): the library decodes it itself --
                                         chunk CRCs and inflate on the calling thread, the row filters and the expansion of palette / sub-byte /
                                         tRNS pictures on the device -- replacing DynamicImage::from_decoder for PNG inputs (src/handler.rs:218-220).
                                         The filtered scanlines cross PCIe: the pixel bytes + height for 8-bit RGB, 3-24 x less for palette and
                                         sub-byte pictures.  Files it does not cover (16-bit samples; Adam7 unless FLGPU_IMG_PNG_ADAM7 is set too):
                                         FLGPU_ERR_UNSUPPORTED (decode on the host); damaged files: FLGPU_ERR_PARSE. */
#define FLGPU_IMG_PNG_ADAM7       256u /* in, beside FLGPU_IMG_PNG_SOURCE (without it: FLGPU_ERR_INVALID_ARG): the caller also hands in Adam7-
                                         interlaced files of up to 8 bits per sample (flgpu_png_info_of_flags says which).  The inflated
                                         stream -- the seven passes' filtered scanlines back to back -- crosses PCIe as it is stored; the
                                         device undoes the row filters pass by pass and puts the passes together while it expands the
                                         samples.  Opt-in, because without it an interlaced file keeps its answer of before
                                         (FLGPU_ERR_UNSUPPORTED) for callers that route on it.  Nothing changes for a non-interlaced file.
                                         16-bit samples stay FLGPU_ERR_UNSUPPORTED; the PNG encoder never writes interlaced files. */
#define FLGPU_IMG_PNG_INFLATE     512u /* in, beside FLGPU_IMG_PNG_SOURCE (without it: FLGPU_ERR_INVALID_ARG), with or without FLGPU_IMG_PNG_ADAM7:
                                         the file's deflate stream is inflated on the device (csrc/fl_inflate.hip).  The calling thread only walks the
                                         container (same CRC checks) and copies the IDAT payloads: the compressed payload crosses PCIe, not the
                                         scanlines.  The device answers "here are the scanlines" or "no"; every "no" is run again with the host
                                         inflate, whose verdict is final, so pixels, status codes and error texts are those of a source without
                                         the bit.  Counters: "png_device_inflates", "png_inflate_retries" (flgpu_debug_get). */
#define FLGPU_IMG_WEBP_SOURCE     64u /* in (src of flgpu_transform / flgpu_transform_batch): data holds a lossless WebP FILE of `capacity` bytes instead
                                         of pixels, width / height / channels say what it decodes to (flgpu_webp_info_of): the library decodes it
                                         itself -- container, prefix codes, LZ77 and colour cache on the calling thread, the predictor, cross-colour,
                                         add-green and colour-indexing transforms on the device -- replacing DynamicImage::from_decoder for WebP
                                         inputs (src/handler.rs:205-220).  The residual picture crosses PCIe: 4 bytes per pixel, 1 / 2 / 4 / 8 x
                                         less for palette pictures.  Lossy and animated files: FLGPU_ERR_UNSUPPORTED (decode on the host);
                                         damaged files: FLGPU_ERR_PARSE. */
#define FLGPU_IMG_VP8_SOURCE      128u /* in (src of flgpu_transform / flgpu_transform_batch): data holds a LOSSY WebP FILE (`VP8 `, with or without VP8X /
                                         ALPH) of `capacity` bytes instead of pixels, width / height / channels say what it decodes to
                                         (flgpu_vp8_info_of): the library decodes it itself -- container, first partition and token partitions
                                         (the boolean coder; a compressed ALPH chunk's prefix codes) on the calling thread; dequantisation, inverse transforms, intra prediction, loop
                                         filter, ALPH filters, chroma up-sampling and YUV -> RGB on the device.  Macroblock records and sparse
                                         levels cross PCIe.  Files it does not cover (flgpu_vp8_info.supported == 0): FLGPU_ERR_UNSUPPORTED
                                         (decode on the host); damaged files: FLGPU_ERR_PARSE.  A source kind of its own: a lossy file handed
                                         in as FLGPU_IMG_WEBP_SOURCE stays FLGPU_ERR_UNSUPPORTED. */
#define FLGPU_IMG_HAS_ALPHA       2u  /* WEBP420: some pixel is not opaque: the picture is WEBP_YUV420A for libwebp, i.e. the A
                                         plane behind V must be handed to WebPEncode too (for opaque pictures it is all 255) */

/* Encoder colour front end to run after the pixel pipeline. */
typedef enum flgpu_front_end {
    FLGPU_FE_NONE = 0,     /* dst = interleaved pixels, out_c channels */
    FLGPU_FE_JFIF444 = 1,  /* dst = Y | Cb | Cr, each plane_w x plane_h (multiples of 8, edge replicated) */
    FLGPU_FE_WEBP420 = 2,  /* dst = Y (w x h) | U | V (each ceil(w/2) x ceil(h/2)) | A (w x h), BT.601 limited range: what
                              libwebp's WebPPictureARGBToYUVA makes of the RGBA picture, alpha-weighted chroma included */
    FLGPU_FE_JPEG = 3,     /* dst = the finished JFIF stream of JpegEncoder::new_with_quality(q).encode_image(&img)
                              (src/handler.rs:274-278): baseline, 3 components, 4:4:4; dst->bytes long */
    FLGPU_FE_PNG = 4,      /* dst = the finished PNG file of PngEncoder (src/handler.rs:264-273): signature, IHDR, IDAT...,
                              IEND; 8-bit samples, colour type 0 / 4 / 2 / 6 for out_c 1 / 2 / 3 / 4, no interlace; row
                              filters by the png crate's adaptive rule; compression from quality (< 50 best, < 85 default,
                              otherwise fast); decodes to exactly the FLGPU_FE_NONE pixels; dst->bytes long */
    /* 5 is not a front end */
    FLGPU_FE_WEBP_LOSSLESS = 6, /* dst = the finished lossless WebP file (RIFF / VP8L) of image's encoder for q == 100
                              (src/handler.rs:286-292): the FLGPU_FE_NONE pixels as img.into_rgba8() gives them,
                              subtract-green, predictor T (L on row 0), one group of prefix codes, runs of the previous pixel;
                              decodes to exactly into_rgba8() of the FLGPU_FE_NONE pixels; out_w, out_h <= 16384;
                              dst->bytes long */
    /* 7 and 8 are not front ends */
    FLGPU_FE_WEBP_LOSSY = 9, /* dst = a finished lossy WebP file (RIFF / VP8, or RIFF / VP8X + ALPH + VP8 where a pixel is not
                              opaque) for the WebP arm below quality 100 (src/handler.rs:293-297): the FLGPU_FE_WEBP420 planes
                              coded as one VP8 key frame -- every macroblock I16, modes by least SSE, one segment, loop filter
                              level 0, default probabilities, quantiser from quality; the alpha plane uncompressed, or with
                              FLGPU_FEO_ALPHA_VP8L in flgpu_params::options (this front end and the seven below) as a VP8L stream
                              wherever that is smaller.  A valid file that decodes to exactly the coder's reconstruction; its
                              bytes are not libwebp's.  out_w, out_h <= 16383 and at most about 21 000 macroblocks (see
                              max_out_bytes); dst->bytes long */
    FLGPU_FE_WEBP_LOSSY_I4 = 10, /* FLGPU_FE_WEBP_LOSSY where a macroblock's luma may also be B_PRED: sixteen 4x4 sub-blocks, each with
                              the one of the ten sub-block predictors that has the least SSE, tried against the macroblock's I16
                              coding and taken when its prediction error plus a penalty from the quantiser is the smaller.
                              Same planes in, same containers, same kind of result; smaller files at equal quality, a slower
                              analysis.  out_w, out_h <= 16383 and at most 5111 macroblocks (the first partition's 19-bit size
                              must hold sixteen sub-block modes per macroblock); dst->bytes long */
    /* 11 is not a front end */
    FLGPU_FE_WEBP_LOSSY_AP = 12, /* FLGPU_FE_WEBP_LOSSY with per-picture coefficient probabilities: the same macroblocks, modes and
                              levels -- the same reconstruction --, but the picture's token-tree branches are counted, a
                              probability is derived per tree node, and the frame header updates the nodes where that pays for
                              its flag and 8 bits; the tokens are coded with the picture's table.  Smaller files, never more
                              than a byte per partition larger; one more kernel launch.  Limits of FLGPU_FE_WEBP_LOSSY;
                              dst->bytes long */
    FLGPU_FE_WEBP_LOSSY_I4_AP = 13, /* FLGPU_FE_WEBP_LOSSY_I4 with per-picture coefficient probabilities, as above.  out_w, out_h <=
                              16383 and at most 5039 macroblocks (the first partition must also hold 1056 updates); dst->bytes
                              long */
    /* 14 and 15 are not front ends */
    FLGPU_FE_WEBP_LOSSY_LF = 16, /* FLGPU_FE_WEBP_LOSSY with a loop filter level picked on the device: the same macroblocks, modes,
                              levels and containers, but the frame header's 6-bit level (normal filter, sharpness 0, no deltas) is
                              the one of four candidates -- 0, ceil(L0 / 2), L0, min(63, L0 + ceil(L0 / 2)), L0 a base level from
                              the quantiser -- whose filtered reconstruction has the least squared error against the source
                              planes (ties: the lowest).  A decoder shows that filtered picture, never a worse one than
                              FLGPU_FE_WEBP_LOSSY's by that measure.  One more kernel launch and three working copies of the
                              reconstruction in scratch.  L0 = 0 (quality 97 and up): FLGPU_FE_WEBP_LOSSY's file byte for byte.
                              Limits and max_out_bytes of FLGPU_FE_WEBP_LOSSY; dst->bytes long */
    FLGPU_FE_WEBP_LOSSY_I4_LF = 17,    /* FLGPU_FE_WEBP_LOSSY_I4 with the loop filter level picked as above; its limits */
    FLGPU_FE_WEBP_LOSSY_AP_LF = 18,    /* FLGPU_FE_WEBP_LOSSY_AP with the loop filter level picked as above; its limits */
    FLGPU_FE_WEBP_LOSSY_I4_AP_LF = 19  /* FLGPU_FE_WEBP_LOSSY_I4_AP with the loop filter level picked as above; its limits */
} flgpu_front_end;

/* content::Format bits (src/content.rs:15-16). */
#define FLGPU_ACCEPT_WEBP 1u
#define FLGPU_ACCEPT_AVIF 2u
/* Not a content::Format bit: the caller wants the library to finish image/png bodies (FLGPU_FE_PNG,
 * FLGPU_RESULT_PNG_STREAM) for PNG inputs that stay PNG.  Without it such requests return pixels, as before. */
#define FLGPU_ENCODE_PNG 0x100u
/* Not a content::Format bit: flgpu_process_png / flgpu_process_png_plan also take Adam7-interlaced files (they hand the file on
 * with FLGPU_IMG_PNG_ADAM7).  Without it such a file is FLGPU_ERR_UNSUPPORTED (as_is aside), as before.  Every other entry point
 * ignores the bit. */
#define FLGPU_DECODE_PNG_ADAM7 0x10000u
/* Not a content::Format bit: flgpu_process_png hands the file on with FLGPU_IMG_PNG_INFLATE (its deflate stream is inflated on the
 * device).  flgpu_process_png_plan ignores it; as_is still never reads the file. */
#define FLGPU_DECODE_PNG_INFLATE 0x100000u
/* Not a content::Format bit: the caller wants the library to finish lossless image/webp bodies (FLGPU_FE_WEBP_LOSSLESS,
 * FLGPU_RESULT_WEBP_STREAM) where the WebP arm runs at quality 100 (src/handler.rs:286-292).  Without it such requests
 * return pixels, as before. */
#define FLGPU_ENCODE_WEBP_LOSSLESS 0x200u
/* Not a content::Format bit: the caller wants flgpu_process_gif to finish the image/gif body (FLGPU_RESULT_GIF_STREAM) where
 * every frame has at most 256 colours -- the exact-palette branch of the reference's GifEncoder (src/handler.rs:355-364).
 * Without it, and for files with a frame above 256 colours (but see FLGPU_ENCODE_GIF_QUANTIZE), the frames return as pixels, as
 * before. */
#define FLGPU_ENCODE_GIF 0x400u
/* Not a content::Format bit: the caller wants the library to finish lossy image/webp bodies (FLGPU_FE_WEBP_LOSSY,
 * FLGPU_RESULT_WEBP_STREAM) where the WebP arm runs below quality 100 (src/handler.rs:293-297) and the output fits the coder's
 * limits.  Without it such requests return the FLGPU_FE_WEBP420 planes, as before. */
#define FLGPU_ENCODE_WEBP_LOSSY 0x800u
/* Not a content::Format bit: together with FLGPU_ENCODE_WEBP_LOSSY, the lossy image/webp bodies come from FLGPU_FE_WEBP_LOSSY_I4
 * where the output fits that front end's limits (FLGPU_FE_WEBP_LOSSY otherwise).  Alone it does nothing. */
#define FLGPU_ENCODE_WEBP_LOSSY_I4 0x1000u
/* Not a content::Format bit: together with FLGPU_ENCODE_WEBP_LOSSY, the lossy image/webp bodies are coded with per-picture
 * coefficient probabilities: FLGPU_FE_WEBP_LOSSY_AP, or with FLGPU_ENCODE_WEBP_LOSSY_I4 as well FLGPU_FE_WEBP_LOSSY_I4_AP where the
 * output fits that front end's limits (FLGPU_FE_WEBP_LOSSY_AP otherwise).  Alone, or with only _I4, it does nothing. */
#define FLGPU_ENCODE_WEBP_LOSSY_PROBS 0x2000u
/* Not a content::Format bit: together with FLGPU_ENCODE_WEBP_LOSSY, the lossy image/webp bodies come from the loop-filtered twin
 * (FLGPU_FE_WEBP_LOSSY_LF, _I4_LF, _AP_LF, _I4_AP_LF) of whichever front end the other bits select, fall-backs included.  Alone, or
 * without FLGPU_ENCODE_WEBP_LOSSY, it does nothing. */
#define FLGPU_ENCODE_WEBP_LOSSY_FILTER 0x4000u
/* Not a content::Format bit: together with FLGPU_ENCODE_WEBP_LOSSY, the lossy image/webp bodies of translucent pictures carry their
 * alpha plane as a VP8L stream wherever that is smaller than the raw plane (FLGPU_FEO_ALPHA_VP8L on whichever lossy front end the
 * other bits select, fall-backs included): the same pixels from every decoder, a file that is never larger.  Opaque pictures keep
 * their bytes.  Alone, or without FLGPU_ENCODE_WEBP_LOSSY, it does nothing. */
#define FLGPU_ENCODE_WEBP_LOSSY_ALPHA 0x20000u
/* Not a content::Format bit: together with FLGPU_ENCODE_WEBP_LOSSY, the lossy image/webp bodies are coded with segment-adaptive
 * quantisers (FLGPU_FEO_SEGMENTS on whichever lossy front end the other bits select, fall-backs included): up to four classes of
 * macroblocks by activity, flat regions at a finer step than texture, as libwebp's own default (four segments) does.  A picture
 * whose classes all come out at the picture's index keeps its file byte for byte.  max_out_bytes grows by the segment header and
 * the ids.  Alone, or without FLGPU_ENCODE_WEBP_LOSSY, it does nothing. */
#define FLGPU_ENCODE_WEBP_LOSSY_SEGMENTS 0x40000u
/* Not a content::Format bit: a JPEG source that stays JPEG (FLGPU_FE_JPEG, FLGPU_RESULT_JPEG_STREAM) is entropy-coded with Huffman
 * tables built from the picture's own symbol counts on the device (FLGPU_FEO_JPEG_OPTIMIZE), as libjpeg's `optimize` switch does:
 * the same quantised coefficients, so every decoder shows the same pixels, in a file that is smaller wherever the picture's tables
 * pay -- and today's file byte for byte where they do not.  max_out_bytes is unchanged.  It does nothing for FLGPU_FE_JFIF444, a
 * negotiated WebP or AVIF, PNG, GIF or as_is. */
#define FLGPU_ENCODE_JPEG_OPTIMIZE 0x80000u
/* Not a content::Format bit: a JPEG source that stays JPEG (FLGPU_FE_JPEG, FLGPU_RESULT_JPEG_STREAM) is coded with 4:2:0 chroma
 * subsampling on the device (FLGPU_FEO_JPEG_420): Cb and Cr at half the resolution in both directions, the standard saving of JPEG
 * files -- about a quarter fewer bytes at quality 75, half at quality 100, for chroma detail most pictures do not show.  The pixels a
 * decoder shows differ from the 4:4:4 file's.  Alone or with FLGPU_ENCODE_JPEG_OPTIMIZE.  It does nothing for FLGPU_FE_JFIF444, a
 * negotiated WebP or AVIF, PNG, GIF or as_is. */
#define FLGPU_ENCODE_JPEG_420 0x200000u
/* Not a content::Format bit: a JPEG source that stays JPEG (FLGPU_FE_JPEG, FLGPU_RESULT_JPEG_STREAM) is written as a progressive
 * file on the device (FLGPU_FEO_JPEG_PROGRESSIVE): the same quantised coefficients in five scans by spectral selection, so every
 * decoder ends at the pixels of the baseline file and shows the whole picture coarsely after the first few hundred bytes.  At
 * ordinary sizes it is also the smallest of the three codings (about 3 % below FLGPU_ENCODE_JPEG_OPTIMIZE on a 300 x 200
 * photograph); a tiny picture grows by its four extra headers, and there is no never-larger fall-back.  With
 * FLGPU_ENCODE_JPEG_OPTIMIZE as well the file is the same.  With FLGPU_ENCODE_JPEG_420 the bit is ignored: the 4:2:0 file stays
 * baseline.  max_out_bytes grows (see flgpu_plan).  It does nothing for FLGPU_FE_JFIF444, a negotiated WebP or AVIF, PNG, GIF or
 * as_is. */
#define FLGPU_ENCODE_JPEG_PROGRESSIVE 0x400000u
/* Not a content::Format bit: together with FLGPU_ENCODE_GIF, a frame above 256 colours is quantised on the device to a local table
 * of at most 256 entries and the file is finished (FLGPU_RESULT_GIF_STREAM) instead of returning as pixels.  The quantiser is the
 * library's own integer rule (a variance-ordered median cut), not the reference's NeuQuant: the file is valid and pinned
 * to the library's model, not to the reference's bytes.  Frames of at most 256 colours keep the exact palette and their bytes.
 * Alone, or without FLGPU_ENCODE_GIF, it does nothing. */
#define FLGPU_ENCODE_GIF_QUANTIZE 0x8000u

/* Output container chosen at src/handler.rs:256-261. */
typedef enum flgpu_out_format { FLGPU_OUT_KEEP = 0, FLGPU_OUT_WEBP = 1, FLGPU_OUT_AVIF = 2 } flgpu_out_format;

/* query::Query, field for field (src/query.rs:4-15); has_* = Option::is_some. */
typedef struct flgpu_query {
    uint8_t has_w, has_h, has_rgb, has_quality, has_crop, has_blur, has_grayscale, has_inverse, has_avif, has_webp;
    uint8_t quality, crop, blur, grayscale, inverse, avif, webp;
    uint8_t reserved;
    uint32_t w, h;
    char rgb[112];      /* NUL terminated copy of the raw `rgb` value (truncated if longer) */
} flgpu_query;

/* Exactly the accessor outputs of query::Query that the pixel pipeline consumes. */
enum flgpu_filter { FLGPU_FILTER_LANCZOS3 = 0, FLGPU_FILTER_NEAREST = 1 };

typedef struct flgpu_params {
    uint32_t has_dims;                 /* Query::dimensions().is_some() */
    uint32_t w, h;
    uint8_t fill_r, fill_g, fill_b;    /* Query::fill_color() */
    uint8_t crop;                      /* Query::cropping() */
    float blur_sigma;                  /* Query::blur(): 0.0 or 10.0..=20.0 */
    uint8_t grayscale, inverse;        /* Query::grayscale(), Query::inverse() */
    uint8_t quality;                   /* Query::quality() (carried for the host encoder) */
    uint8_t front_end;                 /* flgpu_front_end */
    uint8_t orientation;               /* EXIF orientation 1..8 from decoder.orientation() (src/handler.rs:206,221-223); 0 or 1 = none */
    uint8_t filter;                    /* flgpu_filter: Lanczos3 for stills (handler.rs:233,235), Nearest for GIF frames (handler.rs:338,340) */
    uint8_t options;                   /* FLGPU_FEO_* bits (0 = every front end as before); a bit that the front end does not know,
                                          or that is not defined, is ignored */
    uint8_t reserved;
} flgpu_params;

/* flgpu_params::options, the byte that used to be the first of two reserved ones (the struct's size and layout are unchanged).
 * FLGPU_FEO_ALPHA_VP8L: the lossy WebP front ends (FLGPU_FE_WEBP_LOSSY, _I4, _AP, _I4_AP and their _LF twins) write the ALPH chunk
 * of a translucent picture as header byte 0x01 and a VP8L stream -- lossless, no filter, no pre-processing -- iff that payload is
 * strictly smaller than the raw one, which is used otherwise; decided on the device.  Every other front end ignores the bit. */
#define FLGPU_FEO_ALPHA_VP8L 1u
/* FLGPU_FEO_SEGMENTS: the same eight front ends sort the picture's macroblocks into up to four classes by luma activity on the device
 * and code each class at a quantiser index of its own around the one from `quality` (DESIGN.md section 4 states the integer rule):
 * the frame header carries the segment header (absolute values, the frame's filter level in every segment), every macroblock its
 * segment id.  Where the rule finds nothing to separate -- one macroblock, a flat picture, one activity bin, every used class at the
 * picture's index -- the file is the one without the bit, byte for byte.  A picture that fits the front end's limits but not the
 * segmented ones (see max_out_bytes) is coded without the bit.  Every other front end ignores it; alone or with
 * FLGPU_FEO_ALPHA_VP8L. */
#define FLGPU_FEO_SEGMENTS 2u
/* FLGPU_FEO_JPEG_OPTIMIZE, which only FLGPU_FE_JPEG knows: the four DHT segments list only the symbols the picture's scan uses, with
 * length-limited minimum-redundancy codes from their counts (DESIGN.md section 4 states the integer rule; no code is all ones, none
 * longer than 16 bits); SOI, APP0, SOF0, DQT, SOS, the coefficients, their order, padding, stuffing and EOI are FLGPU_FE_JPEG's.  The
 * device compares header + entropy-coded bytes of both codings and writes the picture's tables only if that is strictly smaller;
 * otherwise the file is FLGPU_FE_JPEG's byte for byte.  Every other front end ignores the bit. */
#define FLGPU_FEO_JPEG_OPTIMIZE 4u
/* FLGPU_FEO_JPEG_420, which only FLGPU_FE_JPEG knows (FLGPU_FE_JFIF444 ignores it too): the file is a baseline JPEG with sampling
 * factors 2x2, 1x1, 1x1.  The Y, Cb, Cr bytes of every pixel are FLGPU_FE_JPEG's; the area is out_w x out_h rounded up to multiples of
 * 16, positions past the right or bottom edge repeating the last column or row; Cb and Cr sample (i, j) is
 * (c[2i][2j] + c[2i][2j+1] + c[2i+1][2j] + c[2i+1][2j+1] + 2) >> 2 on those bytes, replicated edge pixels included; transform, quantiser
 * (luma table for Y, chroma table for Cb and Cr), Annex K Huffman tables, padding, stuffing and EOI are FLGPU_FE_JPEG's; one interleaved
 * scan of 16 x 16 MCUs in raster order, each Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr; the header is FLGPU_FE_JPEG's 623 bytes with the
 * sampling byte of SOF0's first component 0x22.  The reference never writes 4:2:0: these bytes are the library's own rule (DESIGN.md
 * section 4), not the crate's.  With FLGPU_FEO_JPEG_OPTIMIZE as well, the counts of this scan go through that option's unchanged rule
 * and decision.  plane_w, plane_h are multiples of 16, chroma_w, chroma_h half of them; out_bytes = 1024 + 3 * plane_w * plane_h / 2;
 * max_out_bytes = 1024 + 2 * 208 * 6 * (plane_w / 16) * (plane_h / 16) -- for a picture of one 8 x 8 block that is LARGER than without
 * the bit (6 units of a 16 x 16 MCU against 3), for every picture whose sides round up the same way it is half. */
#define FLGPU_FEO_JPEG_420 8u
/* FLGPU_FEO_JPEG_PROGRESSIVE, which only FLGPU_FE_JPEG knows (FLGPU_FE_JFIF444 ignores it too): the file is a progressive JPEG
 * (SOF2), 4:4:4, of FLGPU_FE_JPEG's quantised coefficients, by spectral selection only (Ah = Al = 0).  FLGPU_FE_JPEG's first 177
 * bytes (SOI, APP0, SOF0, DQT, DQT) with byte 21 0xC2; scan 1: DC of Y, Cb, Cr interleaved behind DHT(class 0, destination 0) from
 * the Y differences, DHT(0, 1) from Cb + Cr and an SOS of (1, 0x00) (2, 0x10) (3, 0x10), Ss = Se = 0; scans 2-5: Y 1-5, Cb 1-63,
 * Cr 1-63, Y 6-63, one component each, blocks in raster order, each behind a DHT(1, 0) from the scan's own counts and its SOS; an AC
 * scan is coded as T.81 G.1.2.2 says (end-of-band runs across blocks, at most 32,767 blocks each, no restarts); every table is
 * FLGPU_FEO_JPEG_OPTIMIZE's rule; every scan ends as FLGPU_FE_JPEG's (ones to the byte edge, 0xFF stuffed); EOI.  The reference never
 * writes SOF2: these bytes are the library's own rule.  There is no never-larger fall-back.  With
 * FLGPU_FEO_JPEG_OPTIMIZE as well the file is the same, byte for byte.  With FLGPU_FEO_JPEG_420 this bit is ignored and the file is
 * the 4:2:0 one.  max_out_bytes = 1104 + 2 * 216 * 3 * (plane_w / 8) * (plane_h / 8): five headers of at most 1,085 bytes together,
 * EOI, a padding byte per scan, and per unit a DC code of 16 + 11 bits, 63 coefficients of 16 + 10 and a run code of 16 + 14 per AC
 * scan it is in (two for Y) -- 1,725 bits in 216 bytes --, every byte stuffed. */
#define FLGPU_FEO_JPEG_PROGRESSIVE 16u

/* Geometry decided on the host before any pixel is touched. */
typedef struct flgpu_plan {
    uint32_t src_w, src_h;             /* source size after img.apply_orientation() (swapped for EXIF 5..8) */
    uint32_t mid_c;                    /* channels after grayscale/invert */
    uint32_t resampled;                /* 1 if a Lanczos3 pass runs */
    uint32_t resized_w, resized_h;     /* resize_exact target */
    uint32_t crop_x, crop_y;           /* resize_to_fill centre-crop origin */
    uint32_t letterboxed;              /* 1 if overlay onto the fill colour runs (output becomes Rgba8) */
    uint32_t place_x, place_y;         /* overlay offset */
    uint32_t out_w, out_h, out_c;      /* pixel image after letterbox/blur */
    uint32_t plane_w, plane_h;         /* front end luma plane size (FLGPU_FE_JPEG: the coded area, multiples of 8; of 16 with FLGPU_FEO_JPEG_420) */
    uint32_t chroma_w, chroma_h;       /* front end chroma plane size */
    uint64_t pixel_bytes;              /* out_w * out_h * out_c */
    uint64_t out_bytes;                /* bytes the call writes to dst (pixels or planes); for FLGPU_FE_JPEG a planning bound
                                          (about 1 byte per sample) that ordinary pictures stay far below; for FLGPU_FE_PNG
                                          the filtered rows, out_h * (1 + out_w * out_c); for FLGPU_FE_WEBP_LOSSLESS a planning
                                          bound, the Rgba8 bytes 4 * out_w * out_h; for FLGPU_FE_WEBP_LOSSY a planning bound, the
                                          bytes of the FLGPU_FE_WEBP420 planes */
    uint64_t max_out_bytes;            /* FLGPU_FE_JPEG: the worst case of the format (every 8x8 block of every component at its
                                          longest code, every byte stuffed; with FLGPU_FEO_JPEG_420 six blocks per 16x16 MCU, with FLGPU_FEO_JPEG_PROGRESSIVE 216 bytes per unit behind 1104, see there): a dst of this capacity can never be too small, as
                                          JpegEncoder::encode_image into a Vec never fails (src/handler.rs:274-278).
                                          FLGPU_FE_PNG: the worst case of the format, every 32 KB segment of the filtered rows
                                          as stored blocks: 63 + sum over segments of (L + 5 * ceil(L / 65535) + 5 + 12).
                                          FLGPU_FE_WEBP_LOSSLESS: the worst case of the format, at most 60 bits per pixel after
                                          headers under 1 KB: 1024 + ceil(15 * out_w * out_h / 2).
                                          FLGPU_FE_WEBP_LOSSY: the worst case of this coder's files: at most 7 bits per boolean,
                                          19 booleans per coefficient, 384 coefficients and 7 mode booleans per macroblock M =
                                          ceil(w / 16) * ceil(h / 16): 80 + w h + ceil(7 (1126 + 7 M) / 8) + ceil(7 (7296 M + 256) / 8).
                                          Pictures for which a partition's worst case could overflow its size field (19 bits
                                          for the first, 24 for a token partition) are not taken: FLGPU_ERR_UNSUPPORTED from
                                          flgpu_plan_output, the planes from flgpu_process_*.
                                          FLGPU_FE_WEBP_LOSSY_I4: the same with 117 mode booleans per macroblock instead of 7.
                                          FLGPU_FE_WEBP_LOSSY_AP, FLGPU_FE_WEBP_LOSSY_I4_AP: the worst case of the front end each
                                          stands beside plus 7392 bytes, 1056 updates of 8 booleans: 9574 where 1126 stands above.
                                          FLGPU_FE_WEBP_LOSSY_LF, _I4_LF, _AP_LF, _I4_AP_LF: the twin's (the bound is per boolean; the
                                          level's six were counted all along).
                                          All eight with FLGPU_FEO_ALPHA_VP8L: unchanged (w h stands for the raw alpha plane, and a
                                          compressed one is only written where it is smaller).
                                          All eight with FLGPU_FEO_SEGMENTS: 98 booleans of segment header and 2 per macroblock more
                                          in the first partition (1224 + 9 per macroblock where 1126 + 7 stands above); at most
                                          5024 macroblocks with B_PRED, 4953 with B_PRED and updates -- a picture over that is
                                          coded without the bit and keeps the bound without it.
                                          Otherwise equal to out_bytes. */
} flgpu_plan;

#define FLGPU_MAX_DEVICES 8
typedef struct flgpu_config {
    int32_t device;            /* HIP device ordinal; -1 = current device (used when n_devices <= 1) */
    uint32_t max_batch;        /* request-queue flush size PER DEVICE (0 = default 16); a flush also ends at 16 MB of pixel sources
                                  per device (three 1080p buffers: the uploads in front of its first kernel), JPEG files not counted */
    uint32_t flush_timeout_us; /* request-queue flush timer (0 = default 200) */
    uint32_t profile;          /* 1 = bracket kernels with HIP events and report them in flgpu_stats */
    uint32_t queue_lanes;      /* flgpu_transform: batches kept in flight at once PER DEVICE (each lane has its own stream
                                  and scratch, so one batch's PCIe transfers overlap another's kernels); 0 = default: 4 lanes, plus 4 overflow
                                  lanes that only take a full batch that is waiting while those four are busy (more callers than
                                  4 x max_batch); a value of 1..8 = exactly that many lanes */
    uint32_t n_devices;        /* 0 or 1: one GPU (`device`).  2..FLGPU_MAX_DEVICES: ONE context for the GPUs of a node, as
                                  the reference shares one Arc<State> between all its workers (src/main.rs:108-112): every
                                  flushed batch of the request queue and every batch call is split into n_devices contiguous
                                  shards balanced by algorithmic bytes (W*H*C + output bytes), shard k runs on devices[k],
                                  results come back in request order.  An ordinal may repeat (two shards on one GPU). */
    uint32_t use_embedded_profile; /* config `use_embedded_profile` (src/handler.rs:19,446-458): CMYK / YCCK JPEG SOURCES decoded by the
                                      library are converted with their own embedded ICC profile when they carry a usable one */
    uint32_t decode_threads;   /* flgpu_transform with FLGPU_IMG_JPEG_SOURCE: callers that may run the host half of the decoder (Huffman
                                  decoding, ~2 ms of CPU per 1080p file) at the same time; the others wait their turn.  0 = the CPUs this
                                  process may use (cgroup quota / affinity mask): more runnable decoders than CPUs only lengthens every
                                  request's decode -- the reference bounds its in-flight requests the same way (max_clients, src/main.rs:108-110) */
    int32_t devices[FLGPU_MAX_DEVICES];
} flgpu_config;

typedef struct flgpu_stats {
    uint64_t images;              /* images transformed */
    uint64_t batches;             /* kernel batches launched */
    uint64_t queue_flushes;       /* request-queue flushes */
    uint64_t tables_built;        /* weight tables built (cache misses) */
    uint64_t resample_launches;   /* launches of the fused resample kernels (streaming + matrix-pipe) */
    double resample_ms;           /* summed HIP-event time of those launches (profile = 1) */
    uint64_t resample_src_bytes;  /* algorithmic bytes read by those launches */
    uint64_t resample_dst_bytes;  /* algorithmic bytes written by those launches */
    uint64_t generic_launches;    /* launches of the two-pass generic resample kernels (through an LDS tile, or through HBM) */
    uint64_t blur_launches;
    double blur_ms;
    uint64_t frontend_launches;
    double frontend_ms;
    uint64_t cmyk_pixels;         /* pixels converted CMYK -> RGB */
    uint64_t cmyk_tables_baked;   /* device-link tables baked from ICC profiles */
    uint64_t jpeg_sources;        /* FLGPU_IMG_JPEG_SOURCE pictures decoded on the device */
    uint64_t jpeg_file_bytes;     /* their file bytes ... */
    uint64_t jpeg_upload_bytes;   /* ... and what crossed PCIe for them (coefficient blobs) */
    uint64_t mfma_launches;       /* launches of the matrix-pipe kernels (fl_mfma.hip, fl_wtile.hip; the latter also for blurs) */
    uint64_t jpeg_device_huffman; /* of jpeg_sources: files whose entropy-coded segment was decoded on the device too (fl_jpeghuff_dev.hip) */
    uint64_t jpeg_device_huffman_retries; /* ... of which the device gave up on and the host decoded after all */
    uint64_t wtile_launches;      /* of mfma_launches: launches of the window-tile matrix-pipe kernel (fl_wtile.hip: mild ratios, up-scales, blurs) */
} flgpu_stats;

typedef struct flgpu_ctx flgpu_ctx;

/* ---- request model (host only, no device needed) ---------------------- */

/* Parses "w=300&h=200&rgb=32,32,32" (the part after '?', or a whole URI) with
 * the semantics of axum::extract::Query<query::Query>: unknown keys ignored,
 * a known key with an unparsable value is an error.  Returns FLGPU_ERR_PARSE
 * where axum would reject the request with 400. */
int flgpu_query_parse(const char *query_string, flgpu_query *out);
int flgpu_query_dimensions(const flgpu_query *q, uint32_t *w, uint32_t *h); /* 1 = Some */
void flgpu_query_fill_color(const flgpu_query *q, uint8_t *r, uint8_t *g, uint8_t *b);
uint8_t flgpu_query_quality(const flgpu_query *q);
int flgpu_query_cropping(const flgpu_query *q);
float flgpu_query_blur(const flgpu_query *q);
int flgpu_query_grayscale(const flgpu_query *q);
int flgpu_query_inverse(const flgpu_query *q);
int flgpu_query_use_avif(const flgpu_query *q);
int flgpu_query_use_webp(const flgpu_query *q);
int flgpu_query_as_is(const flgpu_query *q);
int flgpu_query_unsupported_scale_size(const flgpu_query *q);

/* Query + content::Format -> pipeline parameters and the output container
 * (src/handler.rs:256-261).  front_end is set to WEBP420 / JFIF444 / NONE from
 * the chosen container and `input_is_jpeg` (JPEG stays JPEG, anything else
 * keeps its own encoder and gets pixels). */
int flgpu_params_from_query(const flgpu_query *q, uint32_t accept_flags, int input_is_jpeg,
                            flgpu_params *params, int *out_format);
/* input_is_jpeg: 0 = no, 1 = JPEG and the caller's encoder wants Y/Cb/Cr planes (FLGPU_FE_JFIF444),
 * 2 = JPEG and the library finishes the stream (FLGPU_FE_JPEG). */

/* Pure function: output geometry for a source of sw x sh x sc. */
int flgpu_plan_output(const flgpu_params *p, uint32_t sw, uint32_t sh, uint32_t sc, flgpu_plan *plan);

/* ---- CMYK / YCCK JPEG sources (reference src/handler.rs:398-493) ------------- */

#define FLGPU_CMYK_GRID 17u          /* nodes per axis of the device-link table (Little CMS default for 4 inputs) */
#define FLGPU_CMYK_INPUT_YCCK 1u     /* pixels are (Y, Cb, Cr, K): run the loop of handler.rs:423-438 first */

/* Replaces create_cmyk_to_rgb_converter / CMYK2RGB::with_icc_profile (src/main.rs:74-76, src/handler.rs:469-488):
 * bakes the CMYK_8 -> sRGB RGB_8, Intent::Perceptual transform of `icc` into the 17^4 table Little CMS itself
 * interpolates, using the system's liblcms2 (dlopen).  FLGPU_ERR_INVALID_ARG = not a usable CMYK profile (the
 * reference's `None`), FLGPU_ERR_UNSUPPORTED = liblcms2 missing on this host. */
int flgpu_set_cmyk_profile(flgpu_ctx *ctx, const uint8_t *icc, uint64_t icc_len);
int flgpu_cmyk_bake_available(void); /* 1 if liblcms2 could be loaded */
/* The same table handed over / read back as grid^4 x 3 u16 (R, G, B), node index ((c*grid + m)*grid + y)*grid + k:
 * for hosts that bake it themselves and for copying rank 0's table to the other GPUs. */
int flgpu_set_cmyk_clut(flgpu_ctx *ctx, uint32_t grid, const uint16_t *rgb_nodes);
int flgpu_get_cmyk_clut(flgpu_ctx *ctx, uint16_t *rgb_nodes, uint64_t capacity_entries, uint32_t *grid);
/* A context that spans several devices bakes the table once and hands it from devices[0] to the others: 2 = by one
 * ncclBroadcast (RCCL over xGMI; one rank per distinct GPU, librccl loaded on demand), 1 = by plain copies (shards sharing
 * a GPU, or no RCCL on the host), 0 = single-device context or no table yet. */
int flgpu_cmyk_distribution(flgpu_ctx *ctx);
/* Self-test of that RCCL path on ONE device: loads librccl as the distribution does, resolves the same five symbols, creates
 * a one-rank communicator (ncclCommInitAll), broadcasts 250,563 bytes out of place as "ncclUint8" between group calls,
 * checks that exactly those bytes arrived, destroys the communicator.  FLGPU_ERR_UNSUPPORTED = no RCCL on this host (the
 * distribution then uses copies).  info (may be NULL): [0] RCCL version, [1] bytes that arrived intact, [2] 1 if nothing was
 * written past them, [3] 1 once the communicator has been destroyed. */
int flgpu_rccl_selftest(int device, uint32_t info[4]);
/* Replaces CMYK2RGB::convert = lcms2 transform_pixels (src/handler.rs:490-492) and, with
 * FLGPU_CMYK_INPUT_YCCK, the YCCK loop in front of it (423-438).  n_pixels x 4 bytes in, n_pixels x 3 bytes out.
 * `embedded_icc` (may be NULL) is the JPEG's own profile when use_embedded_profile is set: it is baked once and
 * cached by content; if it cannot be used the configured profile is (handler.rs:446-458).  With no usable
 * profile at all: FLGPU_ERR_UNSUPPORTED (the reference returns None and decodes the JPEG the ordinary way). */
int flgpu_cmyk_to_rgb(flgpu_ctx *ctx, const uint8_t *cmyk, uint64_t n_pixels, uint8_t *rgb,
                      const uint8_t *embedded_icc, uint64_t icc_len, uint32_t flags);
/* Device-resident variant with the configured profile: d_cmyk 16-byte aligned and readable up to a multiple of 4
 * pixels, d_rgb 4-byte aligned and writable up to a multiple of 4 pixels; returns after enqueueing. */
int flgpu_cmyk_to_rgb_device(flgpu_ctx *ctx, const void *d_cmyk, void *d_rgb, uint64_t n_pixels, uint32_t flags,
                             void *hip_stream);

/* ---- device context ---------------------------------------------------- */

/* Returns NULL on failure; *status (optional) receives the reason. */
flgpu_ctx *flgpu_create(const flgpu_config *cfg, int *status);
void flgpu_destroy(flgpu_ctx *ctx);

/* One image, host memory, blocking.  Thread-safe: concurrent callers are
 * packed into shared kernel launches by the context's request queue. */
int flgpu_transform(flgpu_ctx *ctx, const flgpu_image *src, const flgpu_params *p, flgpu_image *dst);

/* State::process_image after the decoder, as one call (src/handler.rs:198-308 minus decoding and the host-only
 * encoders): `decoded` = DynamicImage::from_decoder's pixels, `exif_orientation` = decoder.orientation() (1..8),
 * `query_string` = the request's query, `accept_flags` = content::Format, `input_format` = what with_guessed_format
 * said.  The outcome is one of flgpu_result_kind:
 *   AS_IS         params.as_is() (handler.rs:202-204): nothing was done, serve the original bytes
 *   JPEG_STREAM   input was JPEG and no other container was negotiated: dst holds the finished "image/jpeg" body
 *   PNG_STREAM    input was PNG, no other container was negotiated and accept_flags has FLGPU_ENCODE_PNG: dst holds the
 *                 finished "image/png" body (handler.rs:264-273), dst->bytes long
 *   WEBP_STREAM   the WebP arm at quality 100 (clamped 1..100, so 255 too; negotiated, or a WebP input that stays WebP) and
 *                 accept_flags has FLGPU_ENCODE_WEBP_LOSSLESS: dst holds the finished lossless "image/webp" body
 *                 (handler.rs:286-292), dst->bytes long; an output wider or taller than 16384 stays PIXELS.
 *                 Also the WebP arm below quality 100 when accept_flags has FLGPU_ENCODE_WEBP_LOSSY and the output is within
 *                 FLGPU_FE_WEBP_LOSSY's limits: dst holds the finished lossy "image/webp" body (handler.rs:293-297)
 *   WEBP_PLANES   lossy WebP was negotiated (handler.rs:286-297) without FLGPU_ENCODE_WEBP_LOSSY, or the output is over that
 *                 coder's limits: dst holds Y | U | V for WebPEncode
 *   PIXELS        everything else (PNG without FLGPU_ENCODE_PNG, AVIF, lossless WebP without FLGPU_ENCODE_WEBP_LOSSLESS, GIF frames, ...): dst holds the DynamicImage pixels for
 *                 the crate's own encoder; *out_format says which container was negotiated
 * Errors: FLGPU_ERR_PARSE where axum answers 400 (bad query, or the size gate of src/main.rs:134-138). */
typedef enum flgpu_input_format { FLGPU_IN_OTHER = 0, FLGPU_IN_JPEG = 1, FLGPU_IN_PNG = 2, FLGPU_IN_WEBP = 3, FLGPU_IN_GIF_FRAME = 4 } flgpu_input_format;
typedef enum flgpu_result_kind { FLGPU_RESULT_AS_IS = 0, FLGPU_RESULT_JPEG_STREAM = 1, FLGPU_RESULT_WEBP_PLANES = 2, FLGPU_RESULT_PIXELS = 3, FLGPU_RESULT_PNG_STREAM = 4,
                                 FLGPU_RESULT_WEBP_STREAM = 5, FLGPU_RESULT_GIF_STREAM = 6 /* flgpu_process_gif with FLGPU_ENCODE_GIF only */ } flgpu_result_kind;
int flgpu_process_image(flgpu_ctx *ctx, const flgpu_image *decoded, uint8_t exif_orientation, const char *query_string,
                        uint32_t accept_flags, int input_format, flgpu_image *dst, flgpu_plan *plan, int *result_kind,
                        int *out_format);
/* Room dst needs for that request (0 for AS_IS); same parsing and errors, no device work. */
int flgpu_process_image_plan(const flgpu_image *decoded, uint8_t exif_orientation, const char *query_string,
                             uint32_t accept_flags, int input_format, flgpu_plan *plan, int *result_kind);

/* ---- JPEG sources (src/handler.rs:205-220: zune-jpeg through the image crate) ----------------------------------------- */
typedef struct flgpu_jpeg_info {
    uint32_t width, height;
    uint32_t components;        /* as stored: 1 (decodes to Luma8), 3 (Rgb8), 4 (CMYK / YCCK) */
    uint32_t channels;          /* of the picture the pipeline sees: 1 or 3 (0 if unsupported).  Four-component files are decoded to
                                   their raw samples and converted to Rgb8 with the configured (or embedded) CMYK profile -- the whole
                                   of convert_jpeg_color_if_needed, src/handler.rs:398-466; without any profile: FLGPU_ERR_UNSUPPORTED */
    uint32_t progressive;       /* SOF2, or any process other than baseline / extended sequential Huffman */
    uint32_t restart_interval;  /* DRI, in MCUs (0 = none) */
    uint32_t h_max, v_max;      /* largest sampling factors: 1x1 = 4:4:4, 2x1 = 4:2:2, 2x2 = 4:2:0 */
    uint32_t exif_orientation;  /* 1..8 from the APP1 Exif segment (decoder.orientation(), src/handler.rs:206); 0 = no tag */
    uint32_t supported;         /* 1 = FLGPU_IMG_JPEG_SOURCE decodes it: 8-bit Huffman-coded baseline / extended sequential (one
                                   scan or several) or progressive (SOF2), 1, 3 or 4 components, every plane at full or half
                                   resolution per direction.  0: arithmetic coding, 12-bit, lossless, hierarchical */
    uint32_t adobe_transform;   /* APP14 transform byte + 1 (0 = no Adobe segment); 4 components: 1 = CMYK, 3 = YCCK */
    uint32_t has_icc_profile;   /* an embedded ICC profile (APP2) is present */
} flgpu_jpeg_info;
/* Header inspection only (no device needed).  FLGPU_ERR_PARSE if the bytes are not a JPEG. */
int flgpu_jpeg_info_of(const uint8_t *jpeg, uint64_t n, flgpu_jpeg_info *info);
/* Decodes a supported JPEG to interleaved pixels in HOST memory at dst->data (capacity >= width*height*channels). */
int flgpu_decode_jpeg(flgpu_ctx *ctx, const uint8_t *jpeg, uint64_t n, flgpu_image *dst);
/* State::process_image for a JPEG input from the file bytes on (src/handler.rs:198-308): header + EXIF orientation,
 * query parsing, size gate, as_is, container negotiation, then decode + pixel pipeline + encode in one device pass.
 * Same outcomes as flgpu_process_image; additionally FLGPU_ERR_UNSUPPORTED for streams the device decoder does not cover
 * (the host then decodes with its own decoder and calls flgpu_process_image). */
int flgpu_process_jpeg(flgpu_ctx *ctx, const uint8_t *jpeg, uint64_t n, const char *query_string, uint32_t accept_flags,
                       flgpu_image *dst, flgpu_plan *plan, int *result_kind, int *out_format);
int flgpu_process_jpeg_plan(const uint8_t *jpeg, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_plan *plan,
                            int *result_kind);

/* ---- PNG sources (src/handler.rs:218-220: the png crate through the image crate, Transformations::EXPAND) --------------- */
typedef struct flgpu_png_info {
    uint32_t width, height;
    uint32_t color_type;        /* as stored: 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA */
    uint32_t bit_depth;         /* as stored: 1, 2, 4, 8 or 16 */
    uint32_t channels;          /* of the picture the pipeline sees (0 if unsupported): colour type 0 -> 1 (Luma8, samples scaled x255 / x85 /
                                   x17), 0 + tRNS -> 2 (LumaA8), 2 -> 3, 2 + tRNS -> 4, 3 -> 3, 3 + tRNS -> 4, 4 -> 2, 6 -> 4 */
    uint32_t interlaced;        /* Adam7 */
    uint32_t has_trns;
    uint32_t supported;         /* 1 = FLGPU_IMG_PNG_SOURCE decodes it; 0: 16-bit samples, Adam7 interlace (but see
                                   flgpu_png_info_of_flags), 2^31 bytes or more */
} flgpu_png_info;
/* Header and chunk inspection only (no device needed): signature, IHDR, PLTE, tRNS, IDAT..., IEND with their CRCs; other ancillary
 * chunks are skipped.  FLGPU_ERR_PARSE if the bytes are not an intact PNG container.  PNG has no orientation (the image crate
 * reports none): the pipeline runs with orientation 1. */
int flgpu_png_info_of(const uint8_t *png, uint64_t n, flgpu_png_info *info);
/* flgpu_png_info_of for a source that will carry src_flags: with FLGPU_IMG_PNG_ADAM7 among them an Adam7 file of up to 8 bits per
 * sample whose seven passes' scanlines and whose pixels stay below 2^31 bytes reports supported = 1 and its channels (interlaced = 1
 * says which kind it is).  Without that flag: flgpu_png_info_of. */
int flgpu_png_info_of_flags(const uint8_t *png, uint64_t n, uint32_t src_flags, flgpu_png_info *info);
/* Decodes a supported PNG to interleaved pixels in HOST memory at dst->data (capacity >= width*height*channels). */
int flgpu_decode_png(flgpu_ctx *ctx, const uint8_t *png, uint64_t n, flgpu_image *dst);
/* flgpu_decode_png (which is this with src_flags 0) for a file handed over with src_flags: FLGPU_IMG_PNG_ADAM7 admits Adam7 files. */
int flgpu_decode_png_flags(flgpu_ctx *ctx, const uint8_t *png, uint64_t n, uint32_t src_flags, flgpu_image *dst);
/* State::process_image for a PNG input from the file bytes on, input_format FLGPU_IN_PNG: query parsing, size gate, as_is, container
 * negotiation, then inflate + unfilter + pixel pipeline (+ PNG encode with FLGPU_ENCODE_PNG) in one pass.  Same outcomes as
 * flgpu_process_image; additionally FLGPU_ERR_UNSUPPORTED for files the decoder does not cover (the host then decodes with its own
 * decoder and calls flgpu_process_image) and FLGPU_ERR_PARSE for damaged ones.  With FLGPU_DECODE_PNG_ADAM7 in accept_flags the
 * decoder covers Adam7-interlaced files too. */
int flgpu_process_png(flgpu_ctx *ctx, const uint8_t *png, uint64_t n, const char *query_string, uint32_t accept_flags,
                      flgpu_image *dst, flgpu_plan *plan, int *result_kind, int *out_format);
int flgpu_process_png_plan(const uint8_t *png, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_plan *plan,
                           int *result_kind);

/* ---- lossless WebP sources (src/handler.rs:205-220: image-webp through the image crate) ----------------------------------- */
typedef struct flgpu_webp_info {
    uint32_t width, height;
    uint32_t channels;          /* of the picture the pipeline sees (0 if unsupported): 4 (Rgba8) if the file announces alpha, else 3 (Rgb8, the
                                   decoded alpha dropped) -- as image 0.25.6 / image-webp report it as far as is known; unpinned */
    uint32_t has_alpha;         /* the VP8L header's alpha bit (simple form), the VP8X alpha flag (extended form) */
    uint32_t extended;          /* the file starts with a VP8X chunk */
    uint32_t animated;          /* VP8X animation flag, ANIM or ANMF */
    uint32_t lossless;          /* the picture is a VP8L chunk */
    uint32_t exif_orientation;  /* 1..8 from the EXIF chunk, 0 = none (the pipeline then runs with 1) */
    uint32_t transforms;        /* bit k = transform type k present: 0 predictor, 1 cross-colour, 2 subtract-green, 3 colour indexing */
    uint32_t color_cache_bits;  /* of the main image, 0 = none */
    uint32_t prefix_groups;     /* code groups of the main image (1 without an entropy image) */
    uint32_t supported;         /* 1 = FLGPU_IMG_WEBP_SOURCE decodes it; 0: lossy VP8 (with or without ALPH), animation */
} flgpu_webp_info;
/* Container, VP8L header, transform headers and the main image's code groups (no device needed).  FLGPU_ERR_PARSE if the bytes are
 * not an intact WebP container or the headers are damaged. */
int flgpu_webp_info_of(const uint8_t *webp, uint64_t n, flgpu_webp_info *info);
/* Decodes a supported WebP to interleaved pixels in HOST memory at dst->data (capacity >= width*height*channels); the EXIF
 * orientation is not applied. */
int flgpu_decode_webp(flgpu_ctx *ctx, const uint8_t *webp, uint64_t n, flgpu_image *dst);
/* State::process_image for a WebP input from the file bytes on, input_format FLGPU_IN_WEBP (so an empty query is as_is), with the
 * file's EXIF orientation: query parsing, size gate, as_is, container negotiation, then entropy decode + inverse transforms + pixel
 * pipeline in one pass (a lossless file as FLGPU_IMG_WEBP_SOURCE, a lossy one as FLGPU_IMG_VP8_SOURCE); with FLGPU_ENCODE_WEBP_LOSSLESS and quality=100 the result is the finished lossless WebP file.  Same
 * outcomes as flgpu_process_image; additionally FLGPU_ERR_UNSUPPORTED for files the decoder does not cover (the host then decodes
 * with its own decoder and calls flgpu_process_image) and FLGPU_ERR_PARSE for damaged ones. */
int flgpu_process_webp(flgpu_ctx *ctx, const uint8_t *webp, uint64_t n, const char *query_string, uint32_t accept_flags,
                       flgpu_image *dst, flgpu_plan *plan, int *result_kind, int *out_format);
int flgpu_process_webp_plan(const uint8_t *webp, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_plan *plan,
                            int *result_kind);

/* ---- lossy WebP sources (src/handler.rs:205-220: image-webp's VP8 decoder through the image crate) ------------------------- */
typedef struct flgpu_vp8_info {
    uint32_t width, height;
    uint32_t channels;          /* of the picture the pipeline sees (0 if unsupported): 4 (Rgba8) if the VP8X header announces alpha, else 3 */
    uint32_t has_alpha;         /* the VP8X alpha flag */
    uint32_t extended;          /* the file starts with a VP8X chunk */
    uint32_t animated;          /* VP8X animation flag, ANIM or ANMF (supported = 0) */
    uint32_t exif_orientation;  /* 1..8 from the EXIF chunk, 0 = none (the pipeline then runs with 1) */
    uint32_t supported;         /* 1 = FLGPU_IMG_VP8_SOURCE decodes it.  0: animation, the colour-space or clamping
                                   bit set, non-zero loop-filter deltas, segment values in delta mode, 2^31 decoded bytes and more */
    uint32_t version;           /* of the frame tag: 0..3 */
    uint32_t segmentation;      /* segmentation enabled */
    uint32_t update_map;        /* ... and the macroblocks carry segment ids */
    uint32_t filter_type;       /* the header's bit: 0 = normal loop filter, 1 = simple */
    uint32_t filter_level;      /* 0..63; 0 = no loop filter */
    uint32_t sharpness;         /* 0..7 */
    uint32_t partitions;        /* token partitions: 1, 2, 4 or 8 */
    uint32_t alpha_compression; /* of the ALPH chunk: 0 = raw, 1 = lossless-coded (0 without a chunk) */
    uint32_t alpha_filter;      /* 0 none, 1 horizontal, 2 vertical, 3 gradient */
    uint32_t segment_quantizers;    /* different quantiser indices among the segments in use (1 without segmentation) */
    uint32_t segment_filter_levels; /* different filter levels among them */
    uint32_t coef_prob_updates; /* coefficient probabilities the header replaces */
    /* from the partitions themselves (0 for an unsupported file): */
    uint32_t macroblocks;
    uint32_t bpred_macroblocks;         /* with sixteen sub-block modes */
    uint32_t skipped_macroblocks;       /* with the skip flag set */
    uint32_t skipped_bpred_macroblocks; /* of those, the ones whose inner edges are filtered all the same */
    uint32_t bmodes_mask;       /* bit k = sub-block mode k seen: 0 DC, 1 TM, 2 VE, 3 HE, 4 RD, 5 VR, 6 LD, 7 VL, 8 HD, 9 HU */
    uint32_t ymodes_mask;       /* bit k = 16x16 mode k seen: 0 DC, 1 V, 2 H, 3 TM */
    uint32_t uvmodes_mask;      /* the same for the chroma modes */
    uint32_t cat6_tokens;       /* tokens of the largest category */
    uint32_t blob_bytes;        /* what crosses PCIe for the file */
    uint32_t reserved[3];
} flgpu_vp8_info;
/* Container, frame header, and -- for a supported file -- the whole first partition and the token partitions (no device needed).
 * FLGPU_ERR_PARSE if the bytes are not an intact lossy WebP file (also: a lossless one) or a partition ends early. */
int flgpu_vp8_info_of(const uint8_t *webp, uint64_t n, flgpu_vp8_info *info);
/* Decodes a supported lossy WebP to interleaved Rgb8 / Rgba8 pixels in HOST memory at dst->data (capacity >= width*height*channels),
 * bit-equal to libwebp's WebPDecodeRGB / WebPDecodeRGBA; the EXIF orientation is not applied.  (flgpu_process_webp and
 * flgpu_process_webp_plan take lossy files too: they go by the chunk type.) */
int flgpu_decode_webp_lossy(flgpu_ctx *ctx, const uint8_t *webp, uint64_t n, flgpu_image *dst);

/* ---- GIF files (src/handler.rs:311-366, process_gif: the gif crate through the image crate) ------------------------------- */
typedef struct flgpu_gif_info {
    uint32_t width, height;     /* the logical screen: the canvas every frame is composited onto (handler.rs:327-333 sees Rgba8 frames of this size) */
    uint32_t frames;
    uint32_t has_global_table;
    uint32_t interlaced_frames;
    uint32_t transparent_frames; /* frames whose graphic control extension names a transparent index */
    uint32_t disposal_mask;     /* bit k = disposal method k occurs */
    uint32_t max_code_size;     /* the largest LZW minimum code size of a frame */
    uint64_t decoded_bytes;     /* frames x width x height x 4: what flgpu_decode_gif writes, and what crosses PCIe on the transform_gif_frames path */
    uint32_t supported;         /* 1 = flgpu_process_gif / flgpu_decode_gif take it; 0: no frames, a frame without area or reaching outside the
                                   canvas, an LZW minimum code size outside 2..8, an index at or beyond its colour table's size, more than 4,096
                                   frames, decoded_bytes above 512 MiB */
    uint32_t reserved;
} flgpu_gif_info;
/* Container and LZW stage of a GIF file (no device needed; the whole file is decoded, since only the indices say whether it is
 * supported).  FLGPU_ERR_PARSE if the file is damaged: bad signature, truncated before the trailer, a zero canvas side, an LZW
 * code beyond the next free entry, fewer indices than a frame has pixels, a frame with neither a local nor a global colour table,
 * an unknown block introducer. */
int flgpu_gif_info_of(const uint8_t *gif, uint64_t n, flgpu_gif_info *info);
/* Decodes a supported GIF to its composited Rgba8 frames -- what GifDecoder::into_frames() yields, handler.rs:315-321 -- one after
 * the other in HOST memory at dst->data (capacity >= decoded_bytes); *frames = their number.  LZW on the calling thread, palette
 * lookup, de-interlacing and the disposal chain on the device.  Delays are not returned (Frame::new at handler.rs:350 drops them
 * too). */
int flgpu_decode_gif(flgpu_ctx *ctx, const uint8_t *gif, uint64_t n, flgpu_image *dst, uint32_t *frames);
/* process_gif from the file bytes on (handler.rs:311-353), input_format FLGPU_IN_GIF_FRAME (so an empty query is as_is, and the
 * per-frame pipeline is Nearest, no blur, no orientation, FE_NONE): query parsing, size gate, as_is, then LZW, compositing and
 * the pipeline of every frame in one pass.  dst->data holds *frames results plan->out_bytes apart (capacity >= frames x
 * out_bytes, see flgpu_process_gif_plan), *result_kind is FLGPU_RESULT_PIXELS, and the host's GifEncoder follows (handler.rs:
 * 355-363).  FLGPU_ERR_UNSUPPORTED / FLGPU_ERR_PARSE as above, both before any device work: the host then decodes with its own
 * decoder (which also substitutes the reference's 1 x 1 grey frames for damaged files; the library does not imitate that) and
 * hands the frames to flgpu_transform_batch.  A GIF is a batch already: it does not travel through flgpu_transform's queue.
 *
 * With FLGPU_ENCODE_GIF in accept_flags the device also writes what GifEncoder::encode_frames writes for frames of at most 256
 * colours (image 0.25.6 over gif 0.13.1, Frame::from_rgba_speed: alpha != 0 becomes 255, the palette is the distinct r, g, b, a
 * tuples in ascending order padded with zeros to 2 .. 256 entries, the transparent index that of the last pixel with alpha 0;
 * GIF89a, no global table, NETSCAPE2.0 loop count 0, every frame a full-canvas image with a local table, disposal 1, delay 0).
 * The per-frame parameters are the same; flgpu_process_gif_plan reports FLGPU_RESULT_GIF_STREAM (what will be attempted),
 * plan->out_bytes stays the pixel bytes of a frame and plan->max_out_bytes = max(out_bytes, worst case of one encoded frame).
 * dst->capacity must be >= 64 + frames x max_out_bytes (FLGPU_ERR_BUFFER_TOO_SMALL otherwise, before any device work), which
 * holds either outcome.  *result_kind says what happened:
 *   GIF_STREAM  dst->data holds the finished file, dst->bytes long, dst->flags has FLGPU_IMG_ENCODED
 *   PIXELS      a frame has more than 256 colours (the reference runs NeuQuant there; the library does not restate it): bytes,
 *               flags and layout exactly as without the bit
 * With FLGPU_ENCODE_GIF_QUANTIZE as well, such a frame gets a local table of at most 256 entries from the library's own quantiser
 * (one entry, behind the others, for all pixels of alpha 0) and the outcome is GIF_STREAM; only a file whose frames have more than
 * 2^22 pixels still returns as PIXELS when a frame exceeds 256 colours.  Capacity and plan are those of FLGPU_ENCODE_GIF.
 * The device decides; the host reads a status record of two words and downloads the file or the pixels, never both.  The LZW
 * stream is not the gif crate's byte for byte (every 2,048 indices it restarts from a clear code, so that segments are coded
 * side by side); it decodes to exactly the frames' indices.  Outputs that are not LumaA8 / Rgba8, sides above 65,535 and
 * files whose worst case reaches 2 GiB are planned and returned as PIXELS. */
int flgpu_process_gif(flgpu_ctx *ctx, const uint8_t *gif, uint64_t n, const char *query_string, uint32_t accept_flags,
                      flgpu_image *dst, flgpu_plan *plan, uint32_t *frames, int *result_kind, int *out_format);
/* The same decisions without a device (container walk only, no LZW): plan and *frames, for sizing dst. */
int flgpu_process_gif_plan(const uint8_t *gif, uint64_t n, const char *query_string, uint32_t accept_flags, flgpu_plan *plan,
                           uint32_t *frames, int *result_kind);

/* Page-locked host memory for sources / results of flgpu_transform (flag them FLGPU_IMG_PINNED): a decoder that
 * writes straight into such a buffer (zune-jpeg's decode_into) saves the 6 MB staging copy of a 1080p request. */
void *flgpu_host_alloc(flgpu_ctx *ctx, uint64_t bytes);
void flgpu_host_free(flgpu_ctx *ctx, void *p);

/* n images, host memory, blocking: staged through pinned buffers, one set of launches. */
int flgpu_transform_batch(flgpu_ctx *ctx, size_t n, const flgpu_image *srcs, const flgpu_params *ps,
                          flgpu_image *dsts);

/* n images already resident in device memory; dsts[i].data are device
 * pointers.  Work is enqueued on `hip_stream` (a hipStream_t; NULL = the
 * context's own stream) and the call returns once it is enqueued; the caller
 * synchronises the stream.  ps may have n entries or, with FLGPU_BATCH_SAME_PARAMS,
 * one entry shared by all images. */
#define FLGPU_BATCH_SAME_PARAMS 1u
int flgpu_transform_batch_device(flgpu_ctx *ctx, size_t n, const flgpu_image *srcs, const flgpu_params *ps,
                                 flgpu_image *dsts, void *hip_stream, uint32_t flags);
/* What only the device knows when flgpu_transform_batch_device returns -- the length of an encoded stream
 * (FLGPU_FE_JPEG, FLGPU_FE_PNG, FLGPU_FE_WEBP_LOSSLESS, FLGPU_FE_WEBP_LOSSY, FLGPU_FE_WEBP_LOSSY_I4, FLGPU_FE_WEBP_LOSSY_AP, FLGPU_FE_WEBP_LOSSY_I4_AP and their four _LF twins: dsts[i].bytes, 0 + FLGPU_ERR_BUFFER_TOO_SMALL if it did not fit dsts[i].capacity) and
 * FLGPU_IMG_HAS_ALPHA of the WebP front end: waits for the most recent device batch of this context and completes
 * the same dsts[] array.  The host-memory entry points do this themselves.
 * It is ALSO where a device-side failure of the batch surfaces: the matrix-pipe resample kernel bounds its waits on LDS
 * hand-offs, and a wait that expired sets the batch's device error word, which this call returns as FLGPU_ERR_DEVICE
 * (the pixels of that batch are then not valid).  Call it once per device batch before using the results, whatever the
 * front end. */
int flgpu_batch_results(flgpu_ctx *ctx, size_t n, flgpu_image *dsts);

/* How a context of n_shards devices splits a batch (pure function, no device needed): shard_of[i] = the shard, hence the
 * device devices[shard_of[i]], that image i runs on -- contiguous runs of images, balanced by algorithmic bytes
 * (W*H*C + flgpu_plan.out_bytes per image).  With a multi-device context the images handed to
 * flgpu_transform_batch_device must be resident on (or peer-accessible from) exactly these devices, and the call then
 * returns only when every shard has finished (`hip_stream` is not used).  shard_bytes (optional, n_shards entries)
 * receives the weight of each shard.  ps has n entries, or one with FLGPU_BATCH_SAME_PARAMS. */
int flgpu_plan_shards(uint32_t n_shards, size_t n, const flgpu_image *srcs, const flgpu_params *ps, uint32_t flags,
                      uint32_t *shard_of, uint64_t *shard_bytes);
/* Devices of a context: returns n_devices (1 for a single-device context) and writes up to `cap` ordinals. */
uint32_t flgpu_devices(flgpu_ctx *ctx, int32_t *devices, uint32_t cap);

/* In-place YCCK -> "CMYK with inverted K" on n_pixels x 4 host bytes: the pointwise loop of
 * convert_jpeg_color_if_needed (src/handler.rs:423-438) that precedes the lcms2 transform.  Blocking. */
int flgpu_ycck_to_cmyk(flgpu_ctx *ctx, uint8_t *raw, uint64_t n_pixels);

/* Read-only device tables (weight tables, row schedules, gamma LUTs) as one blob.
 * Multi-GPU runs build them on rank 0, broadcast the blob over RCCL/xGMI and install
 * it on the other ranks, so every GPU resamples with byte-identical tables.
 *   export: device pointer + size of this context's blob (valid until the next transform call);
 *   copy:   device-to-device copy of the blob into a caller-owned device buffer;
 *   import: overwrite this context's blob with `bytes` from a device buffer; the layout must
 *           match what this context planned locally (same requests prepared in the same order),
 *           otherwise FLGPU_ERR_INVALID_ARG. */
int flgpu_export_tables(flgpu_ctx *ctx, void **device_ptr, uint64_t *bytes);
int flgpu_copy_tables(flgpu_ctx *ctx, void *dst_device, uint64_t capacity, uint64_t *bytes);
int flgpu_import_tables(flgpu_ctx *ctx, const void *src_device, uint64_t bytes);

int flgpu_get_stats(flgpu_ctx *ctx, flgpu_stats *out);
int flgpu_reset_stats(flgpu_ctx *ctx);

/* Test and experiment switches of a context (ABI 6).  The reference shares ONE Arc<State> between all its worker threads
 * (src/main.rs:108-112), so nothing in the library may depend on the process environment after start-up: getenv races setenv in a
 * multi-threaded server, and a stray variable must not change output bytes.  The environment is read exactly once, in flgpu_create
 * (FLGPU_<KEY IN CAPITALS> seeds the switch `key`); afterwards a switch changes only through this call, atomically, for the
 * context, its queue lanes and its device shards.  Keys (csrc/fl_context.h DebugKey): "no_mfma", "force_generic", "no_wtile",
 * "no_luma_mid" (a grey picture on a grey frame is blurred as Rgba8, not as one channel), "wtile_first", "mfma_arith" (0 full width,
 * 1 packed), "force_bands", "no_tile", "no_place4", "host_huffman", "device_huffman_always", "device_huffman_min_bytes",
 * "mfma_spin_limit", "debug_mfma", "debug_jh", "vp8_filter_base" (see flgpu_debug_vp8_filter_costs), "jpeg_optimize_fallback" (1: a
 * FLGPU_FEO_JPEG_OPTIMIZE picture's size comparison always falls against its own tables -- tests reach the fallback branch with it);
 * "reset" restores every default.
 * flgpu_debug_get also reads three counters of the context (its queue lanes and device shards included; flgpu_reset_stats clears
 * them; flgpu_debug_set refuses them): "png_sources" = FLGPU_IMG_PNG_SOURCE pictures decoded, "png_file_bytes" = their file bytes,
 * "png_upload_bytes" = what crossed PCIe for them (per picture a 1,088-byte header + height x (1 + row bytes) of filtered scanlines;
 * for an Adam7 picture the header + the sum over its non-empty passes of pass height x (1 + pass row bytes); for a picture handed over
 * with FLGPU_IMG_PNG_INFLATE the header + its IDAT payloads + 16 bytes of padding), "png_device_inflates" = pictures the inflate kernel
 * inflated, "png_inflate_retries" = pictures it said no to, which were run again with the host inflate;
 * "webp_sources", "webp_file_bytes", "webp_upload_bytes" the same for FLGPU_IMG_WEBP_SOURCE pictures (per picture a 112-byte header,
 * the transforms' sub-images and 4 bytes per pixel of the packed width), and with flgpu_config.profile "webp_predict_ns" /
 * "webp_pointwise_ns" = the HIP-event time of the predictor and the pointwise kernels' launches (complete after flgpu_get_stats);
 * "vp8_sources", "vp8_file_bytes", "vp8_upload_bytes" the same for FLGPU_IMG_VP8_SOURCE pictures (per picture a 128-byte header, 48
 * bytes per macroblock, the levels up to each block's last non-zero one, the raw ALPH plane or a compressed one's lossless blob), with flgpu_config.profile "vp8_decode_ns" =
 * the HIP-event time of their decode kernels;
 * with flgpu_config.profile "webp_lossy_ns" = the HIP-event time of the lossy WebP encoder's launches (FLGPU_FE_WEBP_LOSSY, FLGPU_FE_WEBP_LOSSY_I4, FLGPU_FE_WEBP_LOSSY_AP, FLGPU_FE_WEBP_LOSSY_I4_AP and their four _LF twins);
 * "gif_sources" = GIF files decoded, "gif_frames" = their frames, "gif_file_bytes" = their file bytes, "gif_upload_bytes" = what
 * crossed PCIe for them (the blob below), and with flgpu_config.profile "gif_compose_ns" = the compose kernel's HIP-event time;
 * "gif_encoded" = files FLGPU_ENCODE_GIF finished on the device, "gif_encoded_bytes" = their bytes, "gif_encode_fallbacks" = files
 * it handed back as pixels (a frame above 256 colours), "gif_quantized_frames" = frames above 256 colours that
 * FLGPU_ENCODE_GIF_QUANTIZE gave a table (their files count as "gif_encoded"), and with flgpu_config.profile "gif_encode_ns" = the encode kernels' HIP-event time;
 * "jpeg_optimized" = FLGPU_FEO_JPEG_OPTIMIZE pictures whose file went out with their own tables (not those that fell back to Annex K's);
 * "jpeg_420" = pictures coded with FLGPU_FEO_JPEG_420 (counted on the host when their launches are enqueued);
 * "jpeg_progressive" = pictures coded with FLGPU_FEO_JPEG_PROGRESSIVE (likewise);
 * "blur_wtile_launches", "blur_tile_launches", "blur_generic_launches" = the blur launches (flgpu_stats.blur_launches is their sum)
 * served by the window-tile matrix-pipe kernel, by the f32 LDS-tile kernel and by the generic two passes.
 * Only "no_mfma", "force_generic", "no_wtile", "no_luma_mid", "wtile_first" and "mfma_arith" can change a result, by at most 1 LSB
 * (they pick another resample or blur kernel).  Unknown key: FLGPU_ERR_INVALID_ARG. */
int flgpu_debug_set(flgpu_ctx *ctx, const char *key, int64_t value);
int flgpu_debug_get(flgpu_ctx *ctx, const char *key, int64_t *value);

/* ---- diagnostics (host only; used by the CPU test-suite) ------------------- */

/* The weight table the runtime uploads for one axis (filter 0 = Lanczos3 as used by
 * resize, 1 = Gaussian of `sigma` with support 2*sigma as used by blur): left[o],
 * count[o] for o < out_size and the packed normalised weights (image 0.25.6
 * imageops/sample.rs maths).  *total receives the number of weights; returns
 * FLGPU_ERR_BUFFER_TOO_SMALL if it exceeds weights_cap. */
int flgpu_debug_axis_table(uint32_t in_size, uint32_t out_size, int filter, float sigma, uint32_t *left,
                           uint32_t *count, float *weights, uint64_t weights_cap, uint64_t *total);

/* Row schedule of the streaming kernel for output rows [y0,y1) of a Lanczos3 axis:
 * returns 1 if the fused kernel can run it (<= 8 rows alive per source row), 0 if the
 * generic two-pass kernels are used instead; *max_live receives the peak. */
/* The host half of the JPEG decode front end alone: the coefficient blob flgpu_transform uploads for a
 * FLGPU_IMG_JPEG_SOURCE (csrc/fl_jpegdec.h: header, one u32 word per block = first coefficient << 7 | count, i16
 * coefficients in zig-zag order up to the last non-zero one).  blob == NULL: *used = capacity to provide. */
int flgpu_debug_jpeg_blob(const uint8_t *jpeg, uint64_t n, uint8_t *blob, uint64_t capacity, uint64_t *used);

/* The host half of the PNG decode front end alone (csrc/fl_pngsrc.h): the filtered scanlines flgpu_transform uploads for a
 * FLGPU_IMG_PNG_SOURCE, height x (1 + row bytes) -- the inflated IDAT stream, Adler-32 and filter bytes checked.
 * out == NULL: *used = capacity to provide. */
int flgpu_debug_png_scanlines(const uint8_t *png, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used);
/* The same for a source that carries src_flags (flgpu_debug_png_scanlines is this with 0).  With FLGPU_IMG_PNG_ADAM7, for an
 * interlaced file: the seven passes' filtered scanlines back to back, for each non-empty pass its height x (1 + its row bytes) -- the
 * inflated IDAT stream as it is stored, Adler-32 and every pass row's filter byte checked. */
int flgpu_debug_png_scanlines_flags(const uint8_t *png, uint64_t n, uint32_t src_flags, uint8_t *out, uint64_t capacity, uint64_t *used);
/* The same scanlines exactly as the inflate kernel (FLGPU_IMG_PNG_INFLATE) leaves them, so that a wrong pixel can name its stage: buffers
 * of its own, no batch and NO host re-run -- a device "no" is FLGPU_ERR_PARSE.  out == NULL: *used alone. */
int flgpu_debug_png_inflate_device(flgpu_ctx *ctx, const uint8_t *png, uint64_t n, uint32_t src_flags, uint8_t *out, uint64_t capacity, uint64_t *used);
/* The host twin of that kernel (csrc/fl_inflate_core.h in plain loops over arrays of the kernel's LDS sizes; not the host inflate): pure host,
 * no context.  FLGPU_ERR_PARSE = the device's "no".  stats (optional): [0] deflate blocks, [1] strips, [2] synchronisation rounds,
 * [3] resolution rounds, [4] tokens decoded, [5] of those decoded more than once, [6] / [7] the most synchronisation / resolution rounds of
 * one strip. */
int flgpu_debug_png_inflate_model(const uint8_t *png, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used, uint32_t stats[8]);

/* The host half of the lossless WebP decode front end alone (csrc/fl_webpsrc.h): the blob flgpu_transform uploads for a
 * FLGPU_IMG_WEBP_SOURCE -- WebpBlobHeader, the mode / cross-colour images, the palette, the entropy-decoded residual picture.
 * out == NULL: *used = capacity to provide. */
int flgpu_debug_webp_residuals(const uint8_t *webp, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used);

/* The host half of the lossy WebP decode front end alone (csrc/fl_vp8src.h): the blob flgpu_transform uploads for a
 * FLGPU_IMG_VP8_SOURCE -- Vp8BlobHeader, one 48-byte record per macroblock, the levels up to each block's last non-zero one, the raw
 * ALPH plane or, for a compressed chunk, the lossless decoder's blob (flgpu_debug_webp_residuals describes it).  out == NULL: *used = capacity to provide. */
int flgpu_debug_vp8_blob(const uint8_t *webp, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used);

/* The lossy WebP decoder's planes on the device (csrc/fl_vp8dec.h): Y | U | V padded to whole macroblocks (16 mbw x 16 mbh, then twice
 * 8 mbw x 8 mbh), before (filter == 0) or behind the loop filter, so that a wrong pixel names its stage.  out == NULL: *used =
 * capacity to provide. */
int flgpu_debug_vp8_planes(flgpu_ctx *ctx, const uint8_t *webp, uint64_t n, int filter, uint8_t *out, uint64_t capacity, uint64_t *used);

/* The loop-filtered lossy WebP front ends' choice (csrc/fl_vp8_lf_core.h): one picture (host memory, as for flgpu_transform) through
 * the ordinary launch sequence of params->front_end (FLGPU_FE_WEBP_LOSSY_LF .. FLGPU_FE_WEBP_LOSSY_I4_AP_LF, else
 * FLGPU_ERR_INVALID_ARG), then levels[4] = the candidate levels, costs[4] = the 64-bit squared-error words the filter launch left
 * for them (all 0 where the base level is 0: nothing is evaluated) and *chosen = the level in the file's frame header.
 * flgpu_debug_set(ctx, "vp8_filter_base", v): -1 (the default) takes the base level from the quantiser, 0..63 forces it; candidates
 * and choice are still made on the device; only these four front ends look at it.  Single-device contexts. */
int flgpu_debug_vp8_filter_costs(flgpu_ctx *ctx, const flgpu_image *src, const flgpu_params *params, uint32_t *levels, uint64_t *costs, uint32_t *chosen);

/* The table rule of FLGPU_FEO_JPEG_OPTIMIZE alone, on the host (csrc/fl_jpeg_opt_core.h, the code jpeg_opt_tables_kernel runs): counts[4][256]
 * = the symbol counts of the four tables in DHT order (DC luma, AC luma, DC chroma, AC chroma; each table's sum below 2^32 - 1).  Out:
 * luts[4][256] = length << 16 | code per symbol (0 = unused); dht[1108] / *dht_bytes = the four DHT segments; *optimized = the
 * never-larger decision for these counts (fallback != 0: as with "jpeg_optimize_fallback"), 0 also where the segments would exceed
 * Annex K's.  Needs no device. */
int flgpu_debug_jpeg_optimize_tables(const uint32_t *counts, int fallback, uint32_t *luts, uint8_t *dht, uint32_t *dht_bytes, int *optimized);

/* FLGPU_FEO_JPEG_PROGRESSIVE alone, on the host, in plain loops (csrc/fl_jpeg_prog_core.h, the rules the kernels of fl_jpeg_prog.hip run):
 * coef[3 * nblocks][64] = the quantised coefficients, unit = 3 * block + component, zig-zag order; prefix = the first 177 bytes of
 * FLGPU_FE_JPEG's header.  Out: counts[6][256] = the symbol counts of the six tables in file order (DC luma, DC chroma, the AC tables
 * of scans 2-5, end-of-band run symbols included); the file at `file` if it fits `capacity`, *file_bytes = its length either way
 * (FLGPU_ERR_BUFFER_TOO_SMALL if it does not fit; nothing is written past capacity).  Needs no device. */
int flgpu_debug_jpeg_progressive_scans(const int16_t *coef, uint32_t nblocks, const uint8_t *prefix, uint32_t *counts, uint8_t *file, uint64_t capacity,
                                       uint64_t *file_bytes);

/* The host half of the GIF decode front end alone (csrc/fl_gifsrc.h): the blob flgpu_process_gif uploads, all fields little-endian
 * dwords, offsets in bytes from the blob's start:
 *   header, 32 bytes:       magic "GIF1", canvas width, height, frames, palettes stored, offset of the first palette, offset of the
 *                           first frame's indices, total bytes
 *   one record per frame, 32 bytes each, behind the header: x, y, w, h of the frame's rectangle, disposal method (0..7), interlaced
 *                           flag, palette offset, index offset
 *   the index bytes of every frame, w x h each, rows in the order the file stores them (an interlaced frame's four passes one
 *                           after the other: the device undoes the interlace)
 *   the palettes, 256 dwords each, R | G << 8 | B << 16 | 255 << 24, entries beyond the colour table's size 0; a frame with a
 *                           transparent index has a copy of its table with that entry 0, 0, 0, 0; a frame whose palette equals the
 *                           frame before's, or the global table's plain copy, shares it
 * out == NULL: *used = a capacity that suffices; with out, *used = the blob's bytes. */
int flgpu_debug_gif_blob(const uint8_t *gif, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used);

int flgpu_debug_stream_schedulable(uint32_t in_size, uint32_t out_size, uint32_t y0, uint32_t y1, uint32_t *max_live);
/* Builds the matrix-pipe kernel's tables (csrc/fl_mfma.h) for a source of sw x sh pixels with `channels` interleaved bytes,
 * resized to rw x rh, kept rows [cy, cy+ch) x columns [cx, cx+cw), and checks them on the host against the plain weight
 * tables: returns 1 if the geometry fits the kernel, 0 if not.  info[0..7] = tiles, K-blocks, strips, largest number of
 * distinct horizontal operands of a strip, log2 of the horizontal weight scale, 1 if the short last tile needs the extra
 * pass, weights of the horizontal tables that are missing / wrong / doubled (must be 0), rows of the vertical tables that
 * are wrong (must be 0).  err[0] = largest |f32 weight - (sum of its two f16 terms)| of the vertical tables, err[1] = largest
 * |weight - fixed-point weight| of the horizontal ones.  Needs no device. */
int flgpu_debug_mfma_plan(uint32_t sw, uint32_t sh, uint32_t channels, uint32_t rw, uint32_t rh, uint32_t cx, uint32_t cy,
                          uint32_t cw, uint32_t ch, uint32_t info[8], double err[2]);
/* The same for one of the kernel's two arithmetics (csrc/fl_mfma.h): arith 1 = full width (what the library uses: weights as
 * three f16 terms / three byte digits; flgpu_debug_mfma_plan is this one), 0 = packed (rounds 2-3: two terms / two digits). */
int flgpu_debug_mfma_plan_arith(uint32_t sw, uint32_t sh, uint32_t channels, uint32_t rw, uint32_t rh, uint32_t cx, uint32_t cy,
                                uint32_t cw, uint32_t ch, uint32_t arith, uint32_t info[8], double err[2]);

/* Which items each persistent workgroup of a uniform matrix-pipe launch walks (csrc/fl_batch.cpp assign_items): `pictures` pictures of
 * `strips` strips and `tiles` 16-row output tiles for a launch of `workgroups` workgroups.  job_of / strip_of / tile0_of / tile1_of
 * [capacity] receive picture, strip and tile range of every item in launch order (*nitems of them: pictures left over after the
 * whole rounds are cut into row bands), lists[2 b], lists[2 b + 1] the first item and item count of workgroup b.  Needs no device. */
int flgpu_debug_assign_items(uint32_t pictures, uint32_t strips, uint32_t tiles, uint32_t workgroups, uint32_t capacity, uint32_t *job_of, uint32_t *strip_of,
                             uint32_t *tile0_of, uint32_t *tile1_of, uint32_t *lists, uint32_t *nitems);

const char *flgpu_strerror(int status);
const char *flgpu_last_error(flgpu_ctx *ctx); /* detail of the last FLGPU_ERR_DEVICE on this context */
uint32_t flgpu_abi_version(void);
/* Build provenance: "sources <first 16 hex digits of the SHA-256 over every source and header of the library>; <hipcc version>;
 * arch ...; flags ..." -- compiled in by csrc/Makefile, which also writes fanlin-rs_amd/build_info.json. */
const char *flgpu_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* FANLIN_GPU_H */
