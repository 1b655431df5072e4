// fl_encode.cpp -- the front ends of a batch (fl_encode.h): each format's bytes, limits and scratch, its jobs, launches and result words.
#include <algorithm>
#include <cassert>

#include "fl_context.h"
#include "fl_jpeg_opt_core.h"
#include "fl_jpeg_prog_core.h"

namespace fl {

// (what out_bytes and max_out_bytes are for each front end, and why: flgpu_plan in include/fanlin_gpu.h)
int encode_plan_bytes(const flgpu_params &p, flgpu_plan &plan)
{
    const std::optional<Vp8Variant> vp8 = vp8_variant_of(p.front_end);
    switch (p.front_end) {
    case FLGPU_FE_JFIF444:
    case FLGPU_FE_JPEG:
        if (jpeg_420(p)) { // FLGPU_FEO_JPEG_420: whole 16 x 16 MCUs of six units; a unit's longest code is what it was
            plan.plane_w = (plan.out_w + 15u) & ~15u; plan.plane_h = (plan.out_h + 15u) & ~15u;
            plan.chroma_w = plan.plane_w / 2u; plan.chroma_h = plan.plane_h / 2u;
            plan.out_bytes = 1024ull + 3ull * plan.plane_w * plan.plane_h / 2u;
            plan.max_out_bytes = 1024ull + 2ull * kJpegMaxUnitBytes * 6ull * (plan.plane_w / 16u) * (plan.plane_h / 16u);
            break;
        }
        plan.plane_w = plan.chroma_w = (plan.out_w + 7u) & ~7u;
        plan.plane_h = plan.chroma_h = (plan.out_h + 7u) & ~7u;
        plan.out_bytes = 3ull * plan.plane_w * plan.plane_h;
        if (p.front_end == FLGPU_FE_JFIF444) break;
        // the stream: a planning bound (header + one byte per sample), and the worst case of the encoder in fl_jpeg.hip: header + 2 x 208
        // bytes per 8x8 block and component (every byte stuffed) -- the library's own staging uses it, so a request fails with
        // FLGPU_ERR_BUFFER_TOO_SMALL only if the finished stream really exceeds the caller's dst->capacity
        plan.out_bytes += 1024ull;
        plan.max_out_bytes = 1024ull + 2ull * kJpegMaxUnitBytes * 3ull * (plan.plane_w / 8u) * (plan.plane_h / 8u);
        // FLGPU_FEO_JPEG_PROGRESSIVE: five headers and five padded scans, a longer DC code and a run code per scan a unit is in (see flgpu_plan)
        if (jpeg_progressive(p)) plan.max_out_bytes = kJpegProgFixedBytes + 2ull * kJpegProgMaxUnitBytes * 3ull * (plan.plane_w / 8u) * (plan.plane_h / 8u);
        break;
    case FLGPU_FE_PNG: // the filtered rows; every segment falls back to stored blocks rather than grow (fl_png.h)
        plan.out_bytes = png_filtered_bytes(plan.out_w, plan.out_h, plan.out_c);
        plan.max_out_bytes = png_max_out_bytes(plan.out_bytes);
        break;
    case FLGPU_FE_WEBP_LOSSLESS: // the VP8L header holds 14 bits of width - 1 and of height - 1
        if (plan.out_w > kWebpllMaxSide || plan.out_h > kWebpllMaxSide) return FLGPU_ERR_UNSUPPORTED;
        plan.out_bytes = 4ull * plan.out_w * plan.out_h;
        plan.max_out_bytes = webpll_max_out_bytes(plan.out_w, plan.out_h);
        break;
    case FLGPU_FE_NONE:
        plan.out_bytes = plan.pixel_bytes;
        break;
    default: // FLGPU_FE_WEBP420: Y | U | V | A (the alpha plane is always written; it matters when FLGPU_IMG_HAS_ALPHA comes back); a lossy
        // WebP front end: the same planes (to scratch), then the VP8 coder, unless a size field of the format could overflow (fl_vp8_core.h:
        // one rule over i4, ap and seg; the loop filter adds nothing, the bound is per boolean)
        if (vp8 && !vp8_fits(plan.out_w, plan.out_h, vp8->i4, vp8->ap)) return FLGPU_ERR_UNSUPPORTED;
        plan.plane_w = plan.out_w;
        plan.plane_h = plan.out_h;
        plan.chroma_w = (plan.out_w + 1u) >> 1;
        plan.chroma_h = (plan.out_h + 1u) >> 1;
        plan.out_bytes = vp8_planes_bytes(plan.plane_w, plan.plane_h);
        if (vp8) plan.max_out_bytes = vp8_max_out_bytes(plan.out_w, plan.out_h, vp8->i4, vp8->ap, vp8_segments(p, plan.out_w, plan.out_h));
        break;
    }
    if (plan.max_out_bytes < plan.out_bytes) plan.max_out_bytes = plan.out_bytes;
    return FLGPU_OK;
}

namespace {

// The scratch one picture needs, appended to s, and the limits flgpu_plan_output does not hold a single picture against.
int jpeg_scratch(const flgpu_plan &pl, EncodeScratch &s, bool optimize, bool s420, bool progressive)
{
    if (pl.out_w > 65535u || pl.out_h > 65535u) return FLGPU_ERR_UNSUPPORTED; // SOF0 carries u16 dimensions (the plan of such a picture is valid: refused when it is run)
    // FLGPU_FEO_JPEG_PROGRESSIVE: four records per block, one per AC scan, where the others hold three units
    const size_t blocks = (size_t)(pl.plane_w / 8u) * (pl.plane_h / 8u);
    const size_t units = s420 ? (size_t)(pl.plane_w / 16u) * (pl.plane_h / 16u) * 6u : blocks * (progressive ? 4u : 3u);
    if (units * kJpegMaxUnitBytes * 8 >= ((size_t)1 << 32)) return FLGPU_ERR_UNSUPPORTED; // bit offsets are 32-bit
    s.jpeg_coef += align_up(units * sizeof(JpegUnit), 256);
    s.jpeg_off += align_up((units + 1) * sizeof(uint32_t), 256);
    s.jpeg_raw += align_up(units * kAcWordsPerUnit * sizeof(uint32_t), 256);
    if (optimize) { // FLGPU_FEO_JPEG_OPTIMIZE: the picture's record and its counts; JpegJob::opt_off is a 32-bit word offset
        if ((s.jpeg_opt + jpeg_opt_bytes(units)) / 4u >= ((size_t)1 << 32)) return FLGPU_ERR_UNSUPPORTED;
        s.jpeg_opt += jpeg_opt_bytes(units);
        s.jpeg_opt_pics++;
    }
    if (progressive) { // the picture's record and its counts, likewise
        if ((s.jpeg_prog + jpeg_prog_bytes(blocks)) / 4u >= ((size_t)1 << 32)) return FLGPU_ERR_UNSUPPORTED;
        s.jpeg_prog += jpeg_prog_bytes(blocks);
        s.jpeg_prog_pics++;
    }
    return FLGPU_OK;
}

int png_scratch(const flgpu_plan &pl, EncodeScratch &s)
{
    const uint64_t fb = png_filtered_bytes(pl.out_w, pl.out_h, pl.out_c);
    if ((uint64_t)s.png_rows + pl.out_h >= (1ull << 31) || (uint64_t)s.png_segs + png_segments(fb) >= (1ull << 31)) return FLGPU_ERR_UNSUPPORTED;
    s.png_filt += align_up(fb, 256);
    s.png_rows += pl.out_h;
    s.png_segs += (uint32_t)png_segments(fb);
    return FLGPU_OK;
}

int webpll_scratch(const flgpu_plan &pl, EncodeScratch &s)
{
    const uint64_t npix = (uint64_t)pl.out_w * pl.out_h;
    // (the second limit is no restatement of the plan's side limit: an alpha plane comes here with a lossy WebP picture's sides)
    if ((uint64_t)s.wll_tiles + webpll_tiles(npix) >= (1ull << 31) || webpll_max_out_bytes(pl.out_w, pl.out_h) / 4u >= (1ull << 32))
        return FLGPU_ERR_UNSUPPORTED;
    s.wll_res += align_up(npix * 4u, 256);
    s.wll_tok += align_up(npix * 2u, 256);
    s.wll_stream += align_up(webpll_max_out_bytes(pl.out_w, pl.out_h), 256);
    s.wll_tiles += (uint32_t)webpll_tiles(npix);
    s.wll_pics++;
    return FLGPU_OK;
}

// Lossy WebP: the front end's planes, the reconstruction (whole macroblocks), 400 levels and one record per macroblock, the sizes;
// the I4 variants' pictures also two words of sub-block modes per macroblock, the adaptive-probability variants' a table, the
// loop-filtered variants' four cost words and three working copies of the reconstruction, a segmented picture's record and class map.
void vp8_scratch(const flgpu_plan &pl, EncodeScratch &s, Vp8Variant v, bool seg)
{
    const uint64_t mbs = (uint64_t)vp8_mbs(pl.out_w) * vp8_mbs(pl.out_h);
    if (v.i4) s.vp8_i4_mbs += mbs;
    if (v.ap) s.vp8_ap_pics++;
    if (v.lf) s.vp8_lf += vp8_lf_bytes(vp8_mbs(pl.out_w), vp8_mbs(pl.out_h));
    if (seg) s.vp8_seg += vp8_seg_bytes(mbs);
    s.vp8_planes += align_up(vp8_planes_bytes(pl.out_w, pl.out_h), 256);
    s.vp8_rec += align_up(vp8_rec_bytes(vp8_mbs(pl.out_w), vp8_mbs(pl.out_h)), 256);
    s.vp8_mbs += mbs;
    s.vp8_pics++;
}

// FLGPU_FEO_ALPHA_VP8L, which only the lossy WebP front ends know: the picture also gets the lossless coder's scratch, for its alpha plane
bool vp8_alpha_vp8l(const flgpu_params &p) { return vp8_variant_of(p.front_end) && (p.options & FLGPU_FEO_ALPHA_VP8L); }

// The header every encoded-stream job starts with: the picture it reads, where the stream goes and how much of it fits, and the
// image whose result words it writes (addressed once the descriptor block has its place).
template <class J> J &encoder_job(std::vector<J> &jobs, std::vector<size_t> &image_of, const EncodeInput &x)
{
    J &j = jobs.emplace_back();
    memset(&j, 0, sizeof(j));
    j.src = x.src;
    j.dst = x.dst;
    j.dst_cap = (uint32_t)std::min<uint64_t>(x.dst_cap, 0xffffffffull);
    j.w = x.plan->out_w; j.h = x.plan->out_h; j.c = x.plan->out_c;
    image_of.push_back(x.image);
    return j;
}

// Each encoder's job.  `at` holds the scratch totals of the jobs before this one, i.e. its offsets (encode_build_jobs moves it on).
void add_jpeg_job(flgpu_ctx *c, EncodeJobs &E, const EncodeInput &x, const EncodeScratch &at)
{
    JpegJob &j = encoder_job(E.jjobs, E.jjob_img, x);
    j.units = reinterpret_cast<JpegUnit *>(static_cast<char *>(c->enc.jpeg_coef.p) + at.jpeg_coef);
    j.unit_off = reinterpret_cast<uint32_t *>(static_cast<char *>(c->enc.jpeg_off.p) + at.jpeg_off);
    j.acbits = reinterpret_cast<uint32_t *>(static_cast<char *>(c->enc.jpeg_raw.p) + at.jpeg_raw);
    const uint32_t side = jpeg_420(*x.p) ? 16u : 8u, v = jpeg_variant(*x.p);
    j.bx = x.plan->plane_w / side; j.by = x.plan->plane_h / side;
    j.tab_off = x.jpeg_tab;
    if (jpeg_optimize(*x.p)) j.opt_off = (uint32_t)(at.jpeg_opt / 4u);
    if (jpeg_progressive(*x.p)) j.opt_off = (uint32_t)(at.jpeg_prog / 4u);
    E.jjobs_of[v]++;
    E.jpeg_max_of[v] = std::max(E.jpeg_max_of[v], j.bx * j.by);
}

void add_png_job(flgpu_ctx *c, EncodeJobs &E, const EncodeInput &x, const EncodeScratch &at)
{
    PngJob &j = encoder_job(E.pjobs, E.pjob_img, x);
    j.fbytes = png_filtered_bytes(x.plan->out_w, x.plan->out_h, x.plan->out_c);
    j.filt = static_cast<uint8_t *>(c->enc.png_filt.p) + at.png_filt;
    j.chunks = static_cast<uint8_t *>(c->enc.png_chunks.p) + (size_t)at.png_segs * kPngSegOutBytes;
    j.syms = static_cast<uint16_t *>(c->enc.png_syms.p) + (size_t)at.png_segs * kPngSegBytes;
    j.recs = static_cast<uint32_t *>(c->enc.png_recs.p) + (size_t)at.png_segs * 4u;
    j.row0 = at.png_rows; j.seg0 = at.png_segs; j.nseg = (uint32_t)png_segments(j.fbytes);
    j.level = png_level(x.p->quality);
}

// vj: the alpha-mode job of lossy WebP job `vj`, which reads the plane that job's planes launch writes and leaves its result in
// front of the stream scratch (the stream itself kWebpllAlphaHead bytes in: webpll_max_out_bytes counts 40 header bits that an ALPH
// payload does not have, and the tail of the scratch is alignment)
void add_webpll_job(flgpu_ctx *c, EncodeJobs &E, const EncodeInput &x, const EncodeScratch &at, Vp8Job *vj = nullptr)
{
    WebpJob &j = vj ? encoder_job(E.ajobs, E.ajob_img, x) : encoder_job(E.wjobs, E.wjob_img, x);
    const flgpu_plan &pl = *x.plan;
    uint32_t &tiles = vj ? E.ajob_tiles : E.wjob_tiles;
    j.res = reinterpret_cast<uint32_t *>(static_cast<char *>(c->enc.webpll_res.p) + at.wll_res);
    j.tok = reinterpret_cast<uint16_t *>(static_cast<char *>(c->enc.webpll_tok.p) + at.wll_tok);
    j.tiles = static_cast<WebpllTile *>(c->enc.webpll_tiles.p) + at.wll_tiles;
    j.pic = static_cast<uint32_t *>(c->enc.webpll_pic.p) + (size_t)at.wll_pics * kWebpllPicWords;
    j.stream = reinterpret_cast<uint32_t *>(static_cast<char *>(c->enc.webpll_stream.p) + at.wll_stream);
    j.tile0 = tiles; j.ntiles = (uint32_t)webpll_tiles((uint64_t)pl.out_w * pl.out_h);
    j.stream_words = (uint32_t)(align_up(webpll_max_out_bytes(pl.out_w, pl.out_h), 256) / 4u);
    tiles += j.ntiles;
    if (vj) {
        j.mode = kWebpllModeAlpha;
        j.src = vj->src + (size_t)pl.out_w * pl.out_h + 2u * (size_t)((pl.out_w + 1u) / 2u) * ((pl.out_h + 1u) / 2u); // behind Y, U, V
        j.dst = reinterpret_cast<uint8_t *>(j.stream);
        j.dst_cap = 0; j.c = 1;
        j.stream += kWebpllAlphaHead / 4u; j.stream_words -= kWebpllAlphaHead / 4u;
        vj->alpha = reinterpret_cast<const uint32_t *>(j.dst);
    }
}

// The lossy WebP job reads the planes its own WebP420 front-end job writes to scratch (add_planes_launch with to_vp8).
void add_vp8_job(flgpu_ctx *c, EncodeJobs &E, const EncodeInput &x, const EncodeScratch &at, Vp8Variant v)
{
    Vp8Job &j = encoder_job(E.vjobs, E.vjob_img, x);
    j.src = static_cast<uint8_t *>(c->enc.vp8_planes.p) + at.vp8_planes;
    j.rec = static_cast<uint8_t *>(c->enc.vp8_rec.p) + at.vp8_rec;
    j.lev = static_cast<int16_t *>(c->enc.vp8_lev.p) + at.vp8_mbs * kVp8MbLevels;
    j.info = static_cast<uint32_t *>(c->enc.vp8_info.p) + at.vp8_mbs;
    j.bm = v.i4 ? static_cast<uint32_t *>(c->enc.vp8_bm.p) + at.vp8_i4_mbs * 2u : nullptr;
    j.tab = v.ap ? static_cast<uint8_t *>(c->enc.vp8_tab.p) + (size_t)at.vp8_ap_pics * kVp8TabBytes : nullptr;
    j.sizes = static_cast<uint32_t *>(c->enc.vp8_sizes.p) + (size_t)at.vp8_pics * kVp8SizeWords;
    j.lf = v.lf ? static_cast<uint8_t *>(c->enc.vp8_lf.p) + at.vp8_lf : nullptr;
    j.lf_base = (int32_t)std::max<int64_t>(-1, std::min<int64_t>(63, c->dbg->get(DBG_VP8_FILTER_BASE)));
    j.qi = vp8_quality_index(clamp_quality(x.p->quality));
    const bool seg = vp8_segments(*x.p, j.w, j.h);
    j.seg = seg ? static_cast<uint8_t *>(c->enc.vp8_seg.p) + at.vp8_seg : nullptr;
    E.vjobs_seg += seg;
    E.vjobs_fam[vp8_family(v)]++;
}

// The planar front ends (JFIF444, WebP420): one launch per kind.  to_vp8: the pictures are lossy WebP jobs (E.vjobs from `vjob0`
// on, in the order of pics) and the planes go to the scratch those jobs read.
void add_planes_launch(EncodeJobs &E, uint32_t kind, const std::vector<const EncodeInput *> &pics, bool to_vp8 = false, size_t vjob0 = 0)
{
    FeLaunch F{kind, (uint32_t)E.fjobs.size(), 0, 0, 0, true};
    for (const EncodeInput *x : pics) {
        const flgpu_plan &pl = *x->plan;
        FrontendJob f; memset(&f, 0, sizeof(f));
        f.src = x->src;
        f.dst = to_vp8 ? const_cast<uint8_t *>(E.vjobs[vjob0 + E.fjobs.size() - F.base].src) : x->dst;
        f.w = pl.out_w; f.h = pl.out_h; f.c = pl.out_c;
        f.plane_w = pl.plane_w; f.plane_h = pl.plane_h; f.chroma_w = pl.chroma_w; f.chroma_h = pl.chroma_h;
        if (f.c != 4 || ((uintptr_t)f.src & 3u) || ((uintptr_t)f.dst & 3u)) F.rgba = false;
        if (F.kind == FLGPU_FE_JFIF444) { F.mw = std::max(F.mw, f.plane_w); F.mh = std::max(F.mh, f.plane_h); }
        else { F.mw = std::max(F.mw, f.chroma_w); F.mh = std::max(F.mh, f.chroma_h); }
        E.fjobs.push_back(f);
        E.fjob_img.push_back(x->image);
        F.n++;
    }
    E.fe_launches.push_back(F);
}

} // namespace

int encode_plan_picture(const flgpu_params &p, const flgpu_plan &plan, EncodeScratch &s)
{
    int rc = FLGPU_OK;
    if (p.front_end == FLGPU_FE_JPEG) rc = jpeg_scratch(plan, s, jpeg_optimize(p) && !jpeg_progressive(p), jpeg_420(p), jpeg_progressive(p));
    if (p.front_end == FLGPU_FE_PNG) rc = png_scratch(plan, s);
    if (p.front_end == FLGPU_FE_WEBP_LOSSLESS) rc = webpll_scratch(plan, s);
    if (const auto v = vp8_variant_of(p.front_end)) vp8_scratch(plan, s, *v, vp8_segments(p, plan.out_w, plan.out_h)); // (its limits: encode_plan_bytes)
    if (!rc && vp8_alpha_vp8l(p)) rc = webpll_scratch(plan, s);
    return rc;
}

int encode_reserve(flgpu_ctx *c, const EncodeScratch &sz)
{
    EncodeBuffers &b = c->enc;
    FL_HIP(c, b.jpeg_coef.reserve(sz.jpeg_coef), "JPEG coefficient scratch");
    FL_HIP(c, b.jpeg_off.reserve(sz.jpeg_off), "JPEG offset scratch");
    FL_HIP(c, b.jpeg_raw.reserve(sz.jpeg_raw), "JPEG bit-stream scratch");
    FL_HIP(c, b.jpeg_opt.reserve(sz.jpeg_opt), "JPEG per-picture table scratch");
    FL_HIP(c, b.jpeg_hist.reserve((size_t)sz.jpeg_opt_pics * kJpegOptHistWords * sizeof(uint32_t)), "JPEG symbol counts");
    FL_HIP(c, b.jpeg_prog.reserve(sz.jpeg_prog), "progressive JPEG per-picture scratch");
    FL_HIP(c, b.jpeg_prog_hist.reserve((size_t)sz.jpeg_prog_pics * kJpegProgHistWords * sizeof(uint32_t)), "progressive JPEG symbol counts");
    FL_HIP(c, b.png_filt.reserve(sz.png_filt), "PNG filtered-row scratch");
    FL_HIP(c, b.png_chunks.reserve((size_t)sz.png_segs * kPngSegOutBytes), "PNG chunk scratch");
    FL_HIP(c, b.png_syms.reserve((size_t)sz.png_segs * kPngSegBytes * sizeof(uint16_t)), "PNG symbol scratch");
    FL_HIP(c, b.png_recs.reserve((size_t)sz.png_segs * 4u * sizeof(uint32_t)), "PNG segment records");
    FL_HIP(c, b.webpll_res.reserve(sz.wll_res), "WebP residual scratch");
    FL_HIP(c, b.webpll_tok.reserve(sz.wll_tok), "WebP token scratch");
    FL_HIP(c, b.webpll_tiles.reserve((size_t)sz.wll_tiles * sizeof(WebpllTile)), "WebP tile records");
    FL_HIP(c, b.webpll_pic.reserve((size_t)sz.wll_pics * kWebpllPicWords * sizeof(uint32_t)), "WebP per-picture scratch");
    FL_HIP(c, b.webpll_stream.reserve(sz.wll_stream), "WebP bit-stream scratch");
    FL_HIP(c, b.vp8_planes.reserve(sz.vp8_planes), "lossy WebP plane scratch");
    FL_HIP(c, b.vp8_rec.reserve(sz.vp8_rec), "lossy WebP reconstruction scratch");
    FL_HIP(c, b.vp8_lev.reserve(sz.vp8_mbs * kVp8MbLevels * sizeof(int16_t)), "lossy WebP level scratch");
    FL_HIP(c, b.vp8_info.reserve(sz.vp8_mbs * sizeof(uint32_t)), "lossy WebP macroblock records");
    FL_HIP(c, b.vp8_bm.reserve(sz.vp8_i4_mbs * 2u * sizeof(uint32_t)), "lossy WebP sub-block mode records");
    FL_HIP(c, b.vp8_tab.reserve((size_t)sz.vp8_ap_pics * kVp8TabBytes), "lossy WebP probability tables");
    FL_HIP(c, b.vp8_lf.reserve(sz.vp8_lf), "lossy WebP loop filter scratch");
    FL_HIP(c, b.vp8_seg.reserve(sz.vp8_seg), "lossy WebP segment scratch");
    FL_HIP(c, b.vp8_sizes.reserve((size_t)sz.vp8_pics * kVp8SizeWords * sizeof(uint32_t)), "lossy WebP partition sizes");
    return FLGPU_OK;
}

void encode_build_jobs(flgpu_ctx *c, const std::vector<EncodeInput> &in, EncodeJobs &E)
{
    std::map<uint32_t, std::vector<const EncodeInput *>> groups; // by front end; FLGPU_FE_JPEG: its five variants in jpeg_variant's order
    for (const EncodeInput &x : in) groups[kJpegVariants * x.p->front_end + jpeg_variant(*x.p)].push_back(&x);
    // E.at runs over ALL the jobs in this order: the lossy WebP groups share the lossy WebP scratch, in the families' order, and the
    // lossless WebP files share the lossless coder's with those groups' alpha planes; no other two formats touch the same total
    for (auto &gk : groups) {
        const std::pair<uint32_t, std::vector<const EncodeInput *> &> g{gk.first / kJpegVariants, gk.second};
        const size_t vjob0 = E.vjobs.size();
        const std::optional<Vp8Variant> vp8 = vp8_variant_of(g.first);
        for (const EncodeInput *x : g.second) {
            if (g.first == FLGPU_FE_JPEG) add_jpeg_job(c, E, *x, E.at);
            if (g.first == FLGPU_FE_PNG) add_png_job(c, E, *x, E.at);
            if (g.first == FLGPU_FE_WEBP_LOSSLESS) add_webpll_job(c, E, *x, E.at);
            if (vp8) add_vp8_job(c, E, *x, E.at, *vp8);
            if (vp8_alpha_vp8l(*x->p)) add_webpll_job(c, E, *x, E.at, &E.vjobs.back());
            const int rc = encode_plan_picture(*x->p, *x->plan, E.at); // past this picture, as when the batch was planned ...
            assert(rc == FLGPU_OK);                                    // ... so the limits hold on these totals: they did on the same ones
            (void)rc;
        }
        if (front_end_kind(g.first).out == FE_OUT_PLANES) add_planes_launch(E, g.first, g.second);
        if (vp8) add_planes_launch(E, FLGPU_FE_WEBP420, g.second, true, vjob0);
    }
}

void EncodeJobs::point_results(uint32_t *status)
{
    auto point = [status](auto &jobs, const std::vector<size_t> &image_of, auto word) { for (size_t k = 0; k < jobs.size(); ++k) jobs[k].*word = status + 2 * image_of[k]; };
    point(jjobs, jjob_img, &JpegJob::result);
    point(fjobs, fjob_img, &FrontendJob::status);
    point(pjobs, pjob_img, &PngJob::result);
    point(wjobs, wjob_img, &WebpJob::result);
    point(ajobs, ajob_img, &WebpJob::result);
    point(vjobs, vjob_img, &Vp8Job::result);
}

void EncodeBuffers::release()
{
    for (DeviceBuf *b : {&jpeg_coef, &jpeg_off, &jpeg_raw, &jpeg_opt, &jpeg_hist, &jpeg_prog, &jpeg_prog_hist, &png_filt, &png_chunks, &png_syms, &png_recs, &webpll_res, &webpll_tok, &webpll_tiles, &webpll_pic,
                         &webpll_stream, &vp8_planes, &vp8_rec, &vp8_lev, &vp8_info, &vp8_sizes, &vp8_bm, &vp8_tab, &vp8_lf, &vp8_seg}) b->release();
}

int encode_enqueue(flgpu_ctx *c, const EncodeJobs &E, hipStream_t st)
{
    for (auto &F : E.fe_launches) {
        ProfileScope ps(c, st, 2);
        if (F.kind == FLGPU_FE_JFIF444) FL_HIP(c, launch_jfif444(E.d.fjobs, F.base, F.n, F.mw, F.mh, F.rgba, st), "jfif front end");
        else FL_HIP(c, launch_webp420(E.d.fjobs, c->d_arena, c->gamma_off, F.base, F.n, F.mw, F.mh, F.rgba, st), "webp front end");
        c->stats.frontend_launches++;
    }
    // FLGPU_FE_JPEG: one launch sequence per variant that has jobs.  The _OPTIMIZE variants' records are addressed by the jobs, their
    // counts by the launch: the 4:2:0 pictures' behind the 4:4:4 ones'.
    uint32_t *const jopt = static_cast<uint32_t *>(c->enc.jpeg_opt.p), *const jhist = static_cast<uint32_t *>(c->enc.jpeg_hist.p);
    const bool fallback = c->dbg->on(DBG_JPEG_OPTIMIZE_FALLBACK);
    uint32_t jbase = 0;
    for (uint32_t v = 0; v < kJpegVariants; jbase += E.jjobs_of[v++]) {
        const uint32_t n = E.jjobs_of[v], most = E.jpeg_max_of[v];
        if (!n) continue;
        ProfileScope ps(c, st, 2);
        if (v == 0u) FL_HIP(c, launch_jpeg_encode(E.d.jjobs, c->d_arena, jbase, n, most, st), "JPEG encode");
        if (v == 1u) FL_HIP(c, launch_jpeg_encode_optimized(E.d.jjobs, c->d_arena, jbase, n, most, jopt, jhist, fallback, st), "JPEG encode with per-picture tables");
        if (v == 2u) FL_HIP(c, launch_jpeg_encode_420(E.d.jjobs, c->d_arena, jbase, n, most, st), "JPEG 4:2:0 encode");
        if (v == 3u) FL_HIP(c, launch_jpeg_encode_420_optimized(E.d.jjobs, c->d_arena, jbase, n, most, jopt, jhist + (size_t)E.jjobs_of[1] * kJpegOptHistWords, fallback, st),
                            "JPEG 4:2:0 encode with per-picture tables");
        if (v == kJpegVariantProgressive) FL_HIP(c, launch_jpeg_encode_progressive(E.d.jjobs, c->d_arena, jbase, n, most, static_cast<uint32_t *>(c->enc.jpeg_prog.p),
                                                                                  static_cast<uint32_t *>(c->enc.jpeg_prog_hist.p), st), "progressive JPEG encode");
        if (v == 2u || v == 3u) c->jpeg_420 += n;
        if (v == kJpegVariantProgressive) c->jpeg_progressive += n;
        c->stats.frontend_launches++;
    }
    if (!E.pjobs.empty()) {
        ProfileScope ps(c, st, 2);
        FL_HIP(c, launch_png_encode(E.d.pjobs, (uint32_t)E.pjobs.size(), E.at.png_rows, E.at.png_segs, st), "PNG encode");
        c->stats.frontend_launches++;
    }
    if (!E.wjobs.empty()) {
        ProfileScope ps(c, st, 2);
        FL_HIP(c, launch_webpll_encode(E.d.wjobs, (uint32_t)E.wjobs.size(), E.wjob_tiles, st), "lossless WebP encode");
        c->stats.frontend_launches++;
    }
    if (!E.vjobs.empty()) {
        ProfileScope ps(c, st, 7);
        // the alpha planes' streams: after the planes launch that wrote the planes and the translucency bits, before any frame kernel
        FL_HIP(c, launch_webpll_encode(E.d.ajobs, (uint32_t)E.ajobs.size(), E.ajob_tiles, st, kWebpllModeAlpha), "lossy WebP alpha plane encode");
        FL_HIP(c, launch_vp8_encode(E.d.vjobs, E.vjobs_fam, st, E.vjobs_seg), "lossy WebP encode");
        c->stats.frontend_launches++;
    }
    return FLGPU_OK;
}

int encode_collect(flgpu_ctx *c, uint32_t fe, uint32_t r0, uint32_t r1, flgpu_image &dst)
{
    if (fe == FLGPU_FE_WEBP420 && (r0 & 1u)) dst.flags |= FLGPU_IMG_HAS_ALPHA;
    if (r1 && (r0 & (kVp8ResultAlphaVp8l | kVp8ResultSegments)) && vp8_variant_of(fe)) {
        c->webp_alpha_vp8l += (r0 & kVp8ResultAlphaVp8l) != 0;
        c->webp_lossy_segments += (r0 & kVp8ResultSegments) != 0;
    }
    if (fe == FLGPU_FE_JPEG && r1 && (r0 & FL_JPEG_RESULT_OPTIMIZED)) c->jpeg_optimized++;
    if (!fe_encoded(fe)) return FLGPU_OK;
    dst.bytes = r1;
    if (r1) return FLGPU_OK;
    c->set_error("encoded stream does not fit the destination");
    return FLGPU_ERR_BUFFER_TOO_SMALL;
}

} // namespace fl

// ---- diagnostics -----------------------------------------------------------------------------------------------------------------
// The rule of fl_jpeg_opt_core.h in plain loops (jpeg_opt_tables_serial): what jpeg_opt_tables_kernel computes over a workgroup.
extern "C" int flgpu_debug_jpeg_optimize_tables(const uint32_t *counts, int fallback, uint32_t *luts, uint8_t *dht, uint32_t *dht_bytes, int *optimized)
try {
    if (!counts || !luts || !dht || !dht_bytes || !optimized) return FLGPU_ERR_INVALID_ARG;
    const int on = fl::jpeg_opt_tables_serial(counts, fallback != 0, luts, dht, dht_bytes);
    if (on < 0) return FLGPU_ERR_INVALID_ARG;
    *optimized = on;
    return FLGPU_OK;
} FL_ABI_CATCH

// FLGPU_FEO_JPEG_PROGRESSIVE in plain loops (jpeg_prog_encode_serial): what the kernels of fl_jpeg_prog.hip compute over a batch.
extern "C" int flgpu_debug_jpeg_progressive_scans(const int16_t *coef, uint32_t nblocks, const uint8_t *prefix, uint32_t *counts, uint8_t *file, uint64_t capacity,
                                                  uint64_t *file_bytes)
try {
    if (!coef || !nblocks || !prefix || !counts || !file_bytes || (!file && capacity)) return FLGPU_ERR_INVALID_ARG;
    if (fl::jpeg_prog_encode_serial(coef, nblocks, prefix, counts, file, capacity, file_bytes)) return FLGPU_ERR_INVALID_ARG;
    return *file_bytes <= capacity ? FLGPU_OK : FLGPU_ERR_BUFFER_TOO_SMALL;
} FL_ABI_CATCH

// One picture through the ordinary launch sequence of a loop-filtered lossy WebP front end; then the cost words its filter launch
// left (the picture is the batch's only one, so its scratch is the start of the loop filter scratch) and what every consumer derives from them.
extern "C" int flgpu_debug_vp8_filter_costs(flgpu_ctx *c, const flgpu_image *src, const flgpu_params *p, uint32_t *levels, uint64_t *costs, uint32_t *chosen)
try {
    using namespace fl;
    if (!c || !src || !p || !levels || !costs || !chosen || !c->dbg || !vp8_variant_of(p->front_end).value_or(Vp8Variant{}).lf || !c->shard_ctx.empty()) return FLGPU_ERR_INVALID_ARG;
    flgpu_plan plan;
    if (int rc = flgpu_plan_output(p, src->width, src->height, src->channels, &plan)) return rc;
    std::vector<uint8_t> file(plan.max_out_bytes);
    flgpu_image dst{};
    dst.data = file.data(); dst.capacity = file.size();
    std::lock_guard<std::mutex> g(c->mu);
    if (int rc = run_batch_host(c, 1, src, p, &dst)) return rc;
    FL_HIP(c, hipMemcpy(costs, c->enc.vp8_lf.p, kVp8LfCandidates * sizeof(uint64_t), hipMemcpyDeviceToHost), "lossy WebP filter costs D2H");
    const uint32_t base = vp8_lf_base_of(vp8_quality_index(clamp_quality(p->quality)), (int32_t)std::max<int64_t>(-1, std::min<int64_t>(63, c->dbg->get(DBG_VP8_FILTER_BASE))));
    for (uint32_t k = 0; k < kVp8LfCandidates; ++k) levels[k] = vp8_lf_candidate(base, k);
    *chosen = vp8_lf_choice(base, costs);
    return FLGPU_OK;
} FL_ABI_CATCH
