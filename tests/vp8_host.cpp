// The lossy WebP encoder's host twin, every variant: the functions of fanlin-rs_amd/csrc/fl_vp8_core.h, fl_vp8_i4_core.h,
// fl_vp8_ap_core.h, fl_vp8_lf_core.h and fl_vp8_seg_core.h -- the ones the kernels of fl_vp8.hip call -- run here in plain loops, from
// the planes of FLGPU_FE_WEBP420 (Y | U | V | A) to the finished file: the segment rule (bins, histogram, classes, indices), the
// analysis with each macroblock's steps taken from its class, with --filter per candidate level the decode front end's filter over
// a copy of the reconstruction and the squared error over the visible samples, then the choice, with --adaptive the counting walk
// over every (macroblock, block) item and the rule per table entry, the coder.  No GPU, no library: a program of its own so that it
// can also be built with -fsanitize=address,undefined.
//   vp8_host <width> <height> <quality> <planes.bin> <out.webp> [--translucent] [--i4] [--adaptive] [--filter] [--filter-base N]
//            [--segments] [--recon FILE] [--shown FILE] [--modes FILE] [--stats FILE]
// --filter-base: the base level the candidates are made from, 0..63 (default -1: from the quantiser).  --segments on a picture over the
// segmented limits is dropped, as the library drops FLGPU_FEO_SEGMENTS.
// --recon: the unfiltered reconstruction cropped to the picture, Y (w x h), U, V (cw x ch); --shown: what a decoder shows, likewise.
// --modes: per macroblock 17 bytes, 1 if it is B_PRED and its sixteen sub-block modes (fl_vp8_dtables.h's numbers; 0 if it is not).
// --stats (with --adaptive): the 1056 zero counts and the 1056 one counts (little-endian 32-bit words), then the 1056 probabilities.
// It prints one line:
//   vp8 ok <bytes> bytes, <n> of <n> macroblocks skipped, <n> B_PRED, <n> of 1056 probabilities updated, levels <4> D <4> chosen <level>,
//   segments on <0|1> qi <4> prob <3>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fl_vp8_ap_core.h"
#include "fl_vp8_i4_core.h"
#include "fl_vp8_lf_core.h"
#include "fl_vp8_seg_core.h"

using namespace fl;

struct Options {
    uint32_t w = 0, h = 0, quality = 0;
    bool alpha = false, i4 = false, adaptive = false, filter = false, segments = false;
    int filter_base = -1;
    const char *planes = nullptr, *out = nullptr, *recon = nullptr, *shown = nullptr, *modes = nullptr, *stats = nullptr;
};

static bool read_file(const char *path, std::vector<uint8_t> &v)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t n = std::fread(v.data(), 1, v.size(), f);
    std::fclose(f);
    return n == v.size();
}

static bool write_file(const char *path, const uint8_t *p, size_t n)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const size_t m = std::fwrite(p, 1, n, f);
    return std::fclose(f) == 0 && m == n;
}

// a reconstruction cropped to the picture: Y (w x h), U, V (cw x ch)
static bool write_cropped(const char *path, const Vp8Pic &p, const uint8_t *rec)
{
    std::vector<uint8_t> out;
    const size_t rys = (size_t)p.mbw * 16, rcs = (size_t)p.mbw * 8, rysz = rys * p.mbh * 16, rcsz = rcs * p.mbh * 8;
    for (uint32_t y = 0; y < p.h; ++y) out.insert(out.end(), rec + y * rys, rec + y * rys + p.w);
    for (int pl = 0; pl < 2; ++pl)
        for (uint32_t y = 0; y < p.ch; ++y) out.insert(out.end(), rec + rysz + pl * rcsz + y * rcs, rec + rysz + pl * rcsz + y * rcs + p.cw);
    return write_file(path, out.data(), out.size());
}

// predict, transform, quantise, reconstruct: macroblocks in raster order, every phase over all of its items
static void analyse_i16(Vp8Pic &p)
{
    for (uint32_t mby = 0; mby < p.mbh; ++mby)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) {
            Vp8Mb m;
            vp8_seg_pick(p, (uint64_t)mby * p.mbw + mbx);
            for (uint32_t k = 0; k < kVp8LoadItems; ++k) vp8_phase_load(p, m, mbx, mby, k);
            for (uint32_t k = 0; k < 3; ++k) vp8_phase_dc(m, mbx, mby, k);
            for (uint32_t k = 0; k < kVp8SseItems; ++k) vp8_phase_sse(m, k);
            vp8_phase_modes(m);
            for (uint32_t b = 0; b < 24; ++b) vp8_phase_fdct(m, b);
            vp8_phase_y2(p, m);
            for (uint32_t b = 0; b < 24; ++b) vp8_phase_recon(p, m, mbx, mby, b);
            for (uint32_t k = 0; k <= kVp8MbLevels; ++k) vp8_phase_store(p, m, mbx, mby, k);
        }
}

static void analyse_i4(Vp8Pic &p)
{
    for (uint32_t mby = 0; mby < p.mbh; ++mby)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) {
            Vp8Mb m;
            vp8_seg_pick(p, (uint64_t)mby * p.mbw + mbx);
            for (uint32_t k = 0; k < kVp8LoadItems; ++k) vp8_phase_load(p, m, mbx, mby, k);
            for (uint32_t k = 0; k < 3; ++k) vp8_phase_dc(m, mbx, mby, k);
            for (uint32_t k = 0; k < kVp8SseItems; ++k) vp8_phase_sse(m, k);
            vp8_phase_modes(m);
            // the I4 trial, sub-block by sub-block, unless the penalty alone already exceeds what I16 leaves
            const uint32_t s16 = vp8_i4_s16(m);
            Vp8I4 t;
            bool i4 = false;
            if (vp8_i4_worth_trying(p, s16)) {
                for (uint32_t k = 0; k < kVp8I4BeginItems; ++k) vp8_i4_phase_begin(p, t, mbx, mby, k);
                for (uint32_t s = 0; s < 16; ++s) {
                    for (uint32_t k = 0; k < kVp8I4EdgeItems; ++k) vp8_i4_phase_edges(m, t, s, k);
                    for (uint32_t mi = 0; mi < 10; ++mi) t.sse[mi] = 0;
                    for (uint32_t k = 0; k < kVp8I4PredictItems; ++k) t.sse[k >> 4] += vp8_i4_phase_predict(m, t, s, k);
                    vp8_i4_phase_pick(t, s);
                    for (uint32_t i = 0; i < 16; ++i) vp8_i4_phase_residual(m, t, s, i);
                    for (uint32_t i = 0; i < 4; ++i) vp8_i4_phase_fdct_rows(t, i);
                    for (uint32_t i = 0; i < 4; ++i) vp8_i4_phase_fdct_cols(t, i);
                    for (uint32_t i = 0; i < 16; ++i) vp8_i4_phase_quant(p, t, s, i);
                    for (uint32_t i = 0; i < 4; ++i) vp8_i4_phase_idct_cols(t, i);
                    for (uint32_t i = 0; i < 4; ++i) vp8_i4_phase_idct_rows(t, i);
                    for (uint32_t i = 0; i < 16; ++i) vp8_i4_phase_recon(t, s, i);
                }
                i4 = vp8_i4_wins(p, t, s16);
            }
            if (i4) {
                for (uint32_t k = 0; k < kVp8I4CommitItems; ++k) vp8_i4_phase_commit(p, m, t, mbx, mby, k);
                for (uint32_t b = 16; b < 24; ++b) vp8_phase_fdct(m, b);
                for (uint32_t b = 16; b < 24; ++b) vp8_phase_recon(p, m, mbx, mby, b);
            } else {
                for (uint32_t b = 0; b < 24; ++b) vp8_phase_fdct(m, b);
                vp8_phase_y2(p, m);
                for (uint32_t b = 0; b < 24; ++b) vp8_phase_recon(p, m, mbx, mby, b);
            }
            for (uint32_t k = 0; k < kVp8I4StoreItems; ++k) vp8_i4_phase_store(p, m, t, i4, mbx, mby, k);
        }
}

template <bool I4, bool AP, bool LF> static void code(Vp8Bool &bw, const Vp8Pic &p, uint32_t qi, uint32_t part, uint32_t nparts, uint32_t level)
{
    if (part == 0) vp8_put_first_partition<I4, AP, LF>(bw, p, qi, nparts, level);
    else vp8_put_token_partition<I4>(bw, p, part - 1, nparts);
}

// one candidate: the filter over a copy, in raster order, then the cost
template <bool I4> static uint64_t candidate_cost(const Vp8Pic &p, uint32_t level, std::vector<uint8_t> &copy)
{
    copy.assign(p.rec, p.rec + vp8_rec_bytes(p.mbw, p.mbh));
    if (level) {
        const Vp8DecPic dp = vp8_lf_pic(p, copy.data());
        for (uint32_t mby = 0; mby < p.mbh; ++mby)
            for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) {
                const Vp8MbRecord r = vp8_lf_record<I4>(p, (uint64_t)mby * p.mbw + mbx, level);
                for (uint32_t s = 0; s < kVp8dFilterSteps; ++s)
                    for (uint32_t lane = 0; lane < kVp8dFilterLanes; ++lane) vp8d_filter(dp, r, mbx, mby, s, lane);
            }
    }
    uint64_t sum = 0;
    for (uint32_t i = 0; i < vp8_lf_items(p); ++i) sum += vp8_lf_sq_diff(p, copy.data(), i);
    return sum;
}

template <bool I4, bool AP, bool LF> static int run(Vp8Pic &p, const Options &o, uint32_t qi, const std::vector<uint8_t> &planes)
{
    const uint32_t w = o.w, h = o.h, mbs = p.mbw * p.mbh, nparts = vp8_partitions(p.mbh);
    if (I4) analyse_i4(p); else analyse_i16(p);
    p.q = vp8_quant(qi); // (the picture's again: the loop filter's base level comes from qi)
    uint32_t skipped = 0, bpred = 0;
    for (uint32_t mb = 0; mb < mbs; ++mb) { skipped += vp8_coded<I4>(p, mb) == 0; bpred += I4 && vp8_is_i4(p, mb); }

    // the level: four candidates, each filtered and measured on a copy of its own
    uint32_t level = 0, levels[kVp8LfCandidates] = {0, 0, 0, 0};
    uint64_t D[kVp8LfCandidates] = {0, 0, 0, 0};
    std::vector<uint8_t> copy;
    if (LF) {
        const uint32_t base = vp8_lf_base_of(qi, o.filter_base);
        for (uint32_t k = 0; k < kVp8LfCandidates; ++k) levels[k] = vp8_lf_candidate(base, k);
        if (base)
            for (uint32_t k = 0; k < kVp8LfCandidates; ++k) D[k] = candidate_cost<I4>(p, levels[k], copy);
        level = vp8_lf_choice(base, D);
    }
    candidate_cost<I4>(p, level, copy); // what a decoder will show

    // the statistics: every (macroblock, block) item on its own, as the kernel's threads take them; then the rule per entry
    std::vector<uint8_t> tab(kVp8CoefProb, kVp8CoefProb + kVp8CoefProbs);
    std::vector<uint32_t> cnt(kVp8CountWords, 0);
    uint32_t updates = 0;
    if (AP) {
        Vp8Count sink{p.prob, cnt.data()};
        for (uint32_t k = 0; k < mbs * kVp8MbBlocks; ++k) vp8_ap_count_item<I4>(sink, p, k);
        for (uint32_t i = 0; i < kVp8CoefProbs; ++i) { tab[i] = vp8_ap_decide(i, cnt[i], cnt[kVp8CoefProbs + i]); updates += tab[i] != kVp8CoefProb[i]; }
        p.prob = tab.data();
    }

    // sizes first (the coder only counts), then every partition at its place in the file
    uint32_t size[9] = {0};
    for (uint32_t k = 0; k <= nparts; ++k) {
        Vp8Bool bw;
        code<I4, AP, LF>(bw, p, qi, k, nparts, level);
        size[k] = bw.pos;
    }
    const Vp8Layout L = vp8_layout(w, h, o.alpha, nparts, size);
    if (L.total > vp8_max_out_bytes(w, h, I4, AP, p.seg != nullptr) || size[0] > vp8_part0_max_bytes(mbs, I4, AP, p.seg != nullptr)) {
        std::fprintf(stderr, "vp8_host: the file exceeds its worst case\n");
        return 1;
    }
    std::vector<uint8_t> file(L.total);
    vp8_put_framing(file.data(), L, w, h, o.alpha, nparts, size);
    if (o.alpha) {
        const uint8_t *a = planes.data() + (size_t)w * h + 2ull * p.cw * p.ch;
        for (size_t i = 0; i < (size_t)w * h; ++i) file[L.alph + 9u + i] = a[i];
    }
    for (uint32_t k = 0; k <= nparts; ++k) {
        Vp8Bool bw;
        bw.buf = file.data() + L.part[k];
        code<I4, AP, LF>(bw, p, qi, k, nparts, level);
        if (bw.pos != size[k]) { std::fprintf(stderr, "vp8_host: partition %u changed its size\n", k); return 1; }
    }
    if (!write_file(o.out, file.data(), file.size())) { std::fprintf(stderr, "vp8_host: cannot write the file\n"); return 1; }
    if (o.recon && !write_cropped(o.recon, p, p.rec)) return 1;
    if (o.shown && !write_cropped(o.shown, p, copy.data())) return 1;
    if (o.modes) {
        std::vector<uint8_t> out;
        for (uint32_t mb = 0; mb < mbs; ++mb) {
            const bool i4 = I4 && vp8_is_i4(p, mb);
            out.push_back(i4);
            for (uint32_t b = 0; b < 16; ++b) out.push_back(i4 ? (uint8_t)vp8_bm_nibble(p, mb, b) : 0);
        }
        if (!write_file(o.modes, out.data(), out.size())) return 1;
    }
    if (o.stats) {
        std::vector<uint8_t> out;
        for (uint32_t v : cnt) for (int b = 0; b < 4; ++b) out.push_back((uint8_t)(v >> (8 * b)));
        out.insert(out.end(), tab.begin(), tab.end());
        if (!write_file(o.stats, out.data(), out.size())) return 1;
    }
    Vp8SegRec r{{(uint8_t)qi, (uint8_t)qi, (uint8_t)qi, (uint8_t)qi}, {255, 255, 255}, 0};
    if (p.seg) r = *p.seg;
    std::printf("vp8 ok %u bytes, %u of %u macroblocks skipped, %u B_PRED, %u of 1056 probabilities updated, levels %u %u %u %u D %llu %llu %llu %llu chosen %u, "
                "segments on %u qi %u %u %u %u prob %u %u %u\n",
                L.total, skipped, mbs, bpred, updates, levels[0], levels[1], levels[2], levels[3], (unsigned long long)D[0], (unsigned long long)D[1],
                (unsigned long long)D[2], (unsigned long long)D[3], level, (unsigned)r.on, (unsigned)r.qi[0], (unsigned)r.qi[1], (unsigned)r.qi[2], (unsigned)r.qi[3],
                (unsigned)r.prob[0], (unsigned)r.prob[1], (unsigned)r.prob[2]);
    return 0;
}

static int usage()
{
    std::fprintf(stderr, "usage: vp8_host <width> <height> <quality> <planes.bin> <out.webp> [--translucent] [--i4] [--adaptive] [--filter] [--filter-base N] "
                         "[--segments] [--recon FILE] [--shown FILE] [--modes FILE] [--stats FILE]\n");
    return 2;
}

int main(int argc, char **argv)
{
    if (argc < 6) return usage();
    Options o;
    o.w = (uint32_t)std::atoi(argv[1]); o.h = (uint32_t)std::atoi(argv[2]); o.quality = (uint32_t)std::atoi(argv[3]);
    o.planes = argv[4]; o.out = argv[5];
    for (int k = 6; k < argc; ++k) {
        const char *a = argv[k];
        const auto flag = [&](const char *name, bool &v) { if (std::strcmp(a, name)) return false; v = true; return true; };
        const auto value = [&](const char *name, const char *&v) { if (std::strcmp(a, name) || k + 1 >= argc) return false; v = argv[++k]; return true; };
        const char *base = nullptr;
        if (flag("--translucent", o.alpha) || flag("--i4", o.i4) || flag("--adaptive", o.adaptive) || flag("--filter", o.filter) || flag("--segments", o.segments) ||
            value("--recon", o.recon) || value("--shown", o.shown) || value("--modes", o.modes) || value("--stats", o.stats)) continue;
        if (!value("--filter-base", base)) return usage();
        o.filter_base = std::atoi(base);
    }
    if ((o.stats && !o.adaptive) || (o.filter_base != -1 && !o.filter)) return usage();
    if (!vp8_fits(o.w, o.h, o.i4, o.adaptive) || o.quality < 1 || o.quality > 99 || o.filter_base < -1 || o.filter_base > 63) {
        std::fprintf(stderr, "vp8_host: outside the coder's limits\n");
        return 2;
    }
    const uint32_t w = o.w, h = o.h;
    Vp8Pic p;
    vp8_pic_dims(p, w, h);
    std::vector<uint8_t> planes(2ull * w * h + 2ull * p.cw * p.ch);
    if (!read_file(o.planes, planes)) { std::fprintf(stderr, "vp8_host: cannot read the planes\n"); return 1; }
    const uint32_t mbs = p.mbw * p.mbh, qi = vp8_quality_index(o.quality);
    std::vector<uint8_t> rec(vp8_rec_bytes(p.mbw, p.mbh));
    std::vector<int16_t> lev((size_t)mbs * kVp8MbLevels);
    std::vector<uint32_t> info(mbs), bm(2 * (size_t)mbs);
    p.src = planes.data(); p.rec = rec.data(); p.lev = lev.data(); p.info = info.data(); p.bm = o.i4 ? bm.data() : nullptr;
    p.q = vp8_quant(qi);

    // the segment rule: the bins of the macroblocks, their histogram, the classes and the record
    Vp8SegRec srec;
    std::vector<uint8_t> map(mbs);
    if (o.segments && vp8_fits(w, h, o.i4, o.adaptive, true)) {
        uint32_t hist[kVp8SegBins];
        uint8_t cls[kVp8SegBins];
        vp8_seg_bins(planes.data(), w, h, map.data(), hist);
        vp8_seg_classify(hist, qi, srec, cls);
        for (uint32_t mb = 0; mb < mbs; ++mb) map[mb] = cls[map[mb]];
        p.seg = &srec; p.segmap = map.data();
    }
    // family i4 | adaptive << 1 | filter << 2, the order of launch_vp8_encode's
    static int (*const family[8])(Vp8Pic &, const Options &, uint32_t, const std::vector<uint8_t> &) = {
        run<false, false, false>, run<true, false, false>, run<false, true, false>, run<true, true, false>,
        run<false, false, true>,  run<true, false, true>,  run<false, true, true>,  run<true, true, true>};
    return family[(uint32_t)o.i4 | (uint32_t)o.adaptive << 1 | (uint32_t)o.filter << 2](p, o, qi, planes);
}
