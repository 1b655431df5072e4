// fl_encode.h -- front ends on the way out of a batch (fl_encode.cpp), the counterpart of fl_source.h: which front ends exist and what each
// leaves in dst, the bytes and limits of every format, and the planar / JPEG / PNG / lossless WebP / lossy WebP jobs of one batch behind
// plan / reserve / build / enqueue / collect.  fl_batch.cpp knows a picture's front end only through these.  (GIF output is a batch of
// its own: fl_gifrun.cpp.)  Included by fl_context.h behind DeviceBuf, which EncodeBuffers holds.
#pragma once
#include <vector>

#include "fl_jpeg.h"
#include "fl_kernels.h"
#include "fl_png.h"
#include "fl_vp8.h"
#include "fl_vp8_variant.h"
#include "fl_webpll.h"

namespace fl {

// ---- the format rules, once each ---------------------------------------------------------------------------------------------

// THE list of front ends: what each leaves in dst -- pixels (no front end), planes, or a stream whose length is a result word, known
// once the batch has run -- and what flgpu_process_* calls that.  Every other code is no front end.
enum FeOutput : uint8_t { FE_OUT_PIXELS, FE_OUT_PLANES, FE_OUT_STREAM };
struct FrontEndKind { bool valid; FeOutput out; int result_kind; };
constexpr FrontEndKind front_end_kind(uint32_t fe)
{
    switch (fe) {
    case FLGPU_FE_NONE: return {true, FE_OUT_PIXELS, FLGPU_RESULT_PIXELS};
    case FLGPU_FE_JFIF444: return {true, FE_OUT_PLANES, FLGPU_RESULT_PIXELS}; // (no request of the query layer ends here)
    case FLGPU_FE_WEBP420: return {true, FE_OUT_PLANES, FLGPU_RESULT_WEBP_PLANES};
    case FLGPU_FE_JPEG: return {true, FE_OUT_STREAM, FLGPU_RESULT_JPEG_STREAM};
    case FLGPU_FE_PNG: return {true, FE_OUT_STREAM, FLGPU_RESULT_PNG_STREAM};
    case FLGPU_FE_WEBP_LOSSLESS: return {true, FE_OUT_STREAM, FLGPU_RESULT_WEBP_STREAM};
    default: return {vp8_variant_of(fe).has_value(), FE_OUT_STREAM, FLGPU_RESULT_WEBP_STREAM}; // the eight lossy WebP front ends (fl_vp8_variant.h)
    }
}
constexpr uint32_t fe_image_flags(uint32_t fe)
{
    const FrontEndKind k = front_end_kind(fe);
    return !k.valid ? 0u : k.out == FE_OUT_STREAM ? FLGPU_IMG_ENCODED : k.out == FE_OUT_PLANES ? FLGPU_IMG_FRONTEND_PLANES : 0u;
}
constexpr bool fe_encoded(uint32_t fe) { return fe_image_flags(fe) == FLGPU_IMG_ENCODED; }
static_assert(vp8_family({true, true, true}) + 1u == kVp8Families, "launch_vp8_encode takes one range of jobs per family");

constexpr uint32_t clamp_quality(uint32_t q) { return q < 1u ? 1u : q > 100u ? 100u : q; } // handler.rs:275 quality().clamp(1, 100)

// FLGPU_FEO_SEGMENTS, which only the lossy WebP front ends know: a w x h output is coded with the option unless it fits the front end's
// limits but not the segmented partition 0's -- then it is coded without it (no record, no class map, the unsegmented worst case)
inline bool jpeg_optimize(const flgpu_params &p) { return p.front_end == FLGPU_FE_JPEG && (p.options & FLGPU_FEO_JPEG_OPTIMIZE); } // only FLGPU_FE_JPEG knows the bit
inline bool jpeg_420(const flgpu_params &p) { return p.front_end == FLGPU_FE_JPEG && (p.options & FLGPU_FEO_JPEG_420); }           // likewise
// FLGPU_FEO_JPEG_PROGRESSIVE: a progressive file -- of a 4:4:4 picture; with FLGPU_FEO_JPEG_420 the bit is ignored (include/fanlin_gpu.h)
inline bool jpeg_progressive(const flgpu_params &p) { return p.front_end == FLGPU_FE_JPEG && (p.options & FLGPU_FEO_JPEG_PROGRESSIVE) && !jpeg_420(p); }
// The five launch sequences of FLGPU_FE_JPEG, in the order of their jobs: plain, _OPTIMIZE, 4:2:0, 4:2:0 + _OPTIMIZE, progressive
// (whose tables are the picture's own with or without _OPTIMIZE)
constexpr uint32_t kJpegVariants = 5, kJpegVariantProgressive = 4;
inline uint32_t jpeg_variant(const flgpu_params &p) { return jpeg_progressive(p) ? kJpegVariantProgressive : (jpeg_optimize(p) ? 1u : 0u) + (jpeg_420(p) ? 2u : 0u); }
inline bool vp8_segments(const flgpu_params &p, uint32_t w, uint32_t h)
{
    const std::optional<Vp8Variant> v = vp8_variant_of(p.front_end);
    return v && (p.options & FLGPU_FEO_SEGMENTS) && vp8_fits(w, h, v->i4, v->ap, true);
}

// The end of flgpu_plan_output: with out_w, out_h, out_c and pixel_bytes in place, the front end's planes geometry, out_bytes (a planning
// bound for streams) and max_out_bytes (the format's worst case: a dst of that capacity is never too small), and the format's limits on
// one picture (FLGPU_ERR_UNSUPPORTED).  p.front_end is valid.
int encode_plan_bytes(const flgpu_params &p, flgpu_plan &plan);

// ---- one batch's front-end state -----------------------------------------------------------------------------------------------

// Bytes (or records) of the encoders' scratch; while pictures are added, the running totals are their offsets.
struct EncodeScratch {
    size_t jpeg_coef = 0, jpeg_off = 0, jpeg_raw = 0, jpeg_opt = 0, jpeg_prog = 0, png_filt = 0, wll_res = 0, wll_tok = 0, wll_stream = 0;
    size_t vp8_planes = 0, vp8_rec = 0, vp8_mbs = 0, vp8_i4_mbs = 0, vp8_lf = 0, vp8_seg = 0;
    uint32_t jpeg_opt_pics = 0, jpeg_prog_pics = 0, png_rows = 0, png_segs = 0, wll_tiles = 0, wll_pics = 0, vp8_pics = 0, vp8_ap_pics = 0;
};

// The encoders' scratch on the device, which lives as long as the context.
struct EncodeBuffers {
    DeviceBuf jpeg_coef, jpeg_off, jpeg_raw; // fl_jpeg.hip: unit records, bit offsets, AC bits past a record
    DeviceBuf jpeg_opt, jpeg_hist;           // fl_jpeg_opt.hip, pictures with FLGPU_FEO_JPEG_OPTIMIZE only: their records (tables, header, DC terms), their AC symbol counts
    DeviceBuf jpeg_prog, jpeg_prog_hist;     // fl_jpeg_prog.hip, pictures with FLGPU_FEO_JPEG_PROGRESSIVE only: their records (tables, headers, DC terms, runs), their AC scans' symbol counts
    DeviceBuf png_filt, png_chunks, png_syms, png_recs; // fl_png.hip: filtered rows, segment chunks, symbols, records
    DeviceBuf webpll_res, webpll_tok, webpll_tiles, webpll_pic, webpll_stream; // fl_webpll.hip: residuals, tokens, tile records, per-picture words, bit streams
    DeviceBuf vp8_planes, vp8_rec, vp8_lev, vp8_info, vp8_sizes, vp8_bm, vp8_tab, vp8_lf, vp8_seg; // fl_vp8.hip: the front end's planes, reconstruction, levels, macroblock records, partition sizes, the I4 variants' sub-block modes, the adaptive-probability variants' tables, the loop-filtered variants' cost words and working copies, the segmented pictures' records and class maps
    void release();
};

// What encode_build_jobs needs of one picture that has a front end.
struct EncodeInput {
    const uint8_t *src; // the picture the front end reads: the blur's output, else stage 1's
    uint8_t *dst; uint64_t dst_cap; // the caller's destination and its capacity
    const flgpu_plan *plan; const flgpu_params *p;
    uint32_t jpeg_tab;  // FLGPU_FE_JPEG: arena offset of its header and quantisation tables
    size_t image;       // its index in the batch: addresses its result words
};

struct FeLaunch { uint32_t kind, base, n, mw, mh; bool rgba; };

// The batch's front-end jobs and the planes launches.  The arrays travel in the batch's descriptor block.
struct EncodeJobs {
    std::vector<FrontendJob> fjobs;
    std::vector<JpegJob> jjobs;
    std::vector<PngJob> pjobs;
    std::vector<WebpJob> wjobs;
    std::vector<WebpJob> ajobs; // the alpha-mode jobs of the lossy WebP pictures that carry FLGPU_FEO_ALPHA_VP8L, in the order of vjobs
    uint32_t wjob_tiles = 0, ajob_tiles = 0; // tiles of each list: a launch numbers its own
    std::vector<Vp8Job> vjobs;
    uint32_t vjobs_fam[kVp8Families] = {0, 0, 0, 0, 0, 0, 0, 0}; // how many of them each family has; the families follow one another (vp8_family)
    uint32_t vjobs_seg = 0; // how many of them are coded with FLGPU_FEO_SEGMENTS (vp8_segments): vp8_segment_kernel launches iff any is
    std::vector<size_t> fjob_img, jjob_img, pjob_img, wjob_img, ajob_img, vjob_img; // image of every job
    // jjobs holds the five variants one after the other (jpeg_variant): how many jobs each has, and the largest bx * by among them
    // (blocks; MCUs for the two 4:2:0 variants).  Each variant has a launch sequence of its own.
    uint32_t jjobs_of[kJpegVariants] = {0, 0, 0, 0, 0}, jpeg_max_of[kJpegVariants] = {0, 0, 0, 0, 0};
    std::vector<FeLaunch> fe_launches;
    EncodeScratch at; // the scratch totals of the jobs so far, i.e. the next job's offsets; once all are built, the batch's totals
    struct { const FrontendJob *fjobs; const JpegJob *jjobs; const PngJob *pjobs; const WebpJob *wjobs; const WebpJob *ajobs; const Vp8Job *vjobs; } d{}; // the arrays' device copies

    // The arrays' regions of the descriptor block (see desc_regions): f(array, device pointer) for the two that precede the matrix-pipe
    // items, and for the four at the block's end.
    template <class F> void head_regions(F &&f) { f(fjobs, d.fjobs); f(jjobs, d.jjobs); }
    template <class F> void tail_regions(F &&f) { f(pjobs, d.pjobs); f(wjobs, d.wjobs); f(ajobs, d.ajobs); f(vjobs, d.vjobs); }
    // Points every job at its image's two result words in `status` (the device copy of the batch's result words).
    void point_results(uint32_t *status);
};

// ---- what fl_batch.cpp calls, in a batch's order ---------------------------------------------------------------------------------

// Planning: the scratch picture (p, plan) needs, appended to s, and the limits that hold for the batch's totals or are not flgpu_plan_output's.
int encode_plan_picture(const flgpu_params &p, const flgpu_plan &plan, EncodeScratch &s);
int encode_reserve(flgpu_ctx *c, const EncodeScratch &sizes);
// The jobs of the pictures `in` (in batch order): grouped by front end in ascending code (FLGPU_FE_JPEG: five groups, jpeg_variant,
// the plain pictures first), batch order inside a group; a job's offsets
// into the scratch are the totals of the jobs before it.  And the planes launches, one per planar kind and one per lossy WebP group.
void encode_build_jobs(flgpu_ctx *c, const std::vector<EncodeInput> &in, EncodeJobs &E);
// Planar front ends, JPEG, PNG, lossless WebP, lossy WebP, in that order.
int encode_enqueue(flgpu_ctx *c, const EncodeJobs &E, hipStream_t st);
// What the caller gets back at once for a picture of front end fe (an encoded stream's length is a result word: flgpu_batch_results) ...
inline void encode_dst_header(uint32_t fe, const flgpu_plan &plan, flgpu_image &dst) { dst.flags = fe_image_flags(fe); dst.bytes = dst.flags == FLGPU_IMG_ENCODED ? 0 : plan.out_bytes; }
// ... and what its result words (r0 flags, r1 stream bytes) add once the batch has run.  FLGPU_ERR_BUFFER_TOO_SMALL: the stream did not fit.
int encode_collect(flgpu_ctx *c, uint32_t fe, uint32_t r0, uint32_t r1, flgpu_image &dst);

} // namespace fl
