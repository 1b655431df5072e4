// The host twin of the lossy WebP encoder with FLGPU_FEO_SEGMENTS: the functions of fanlin-rs_amd/csrc/fl_vp8_core.h, fl_vp8_i4_core.h,
// fl_vp8_ap_core.h, fl_vp8_lf_core.h and fl_vp8_seg_core.h -- the ones the kernels of fl_vp8.hip call -- run here in plain loops, from
// the planes of FLGPU_FE_WEBP420 (Y | U | V | A) to the finished file: the segment rule (bins, histogram, classes, indices), the
// analysis with each macroblock's steps taken from its class, for a loop-filtered family the level's choice, the probability table
// of an adaptive family, the coder with the segment header and the ids.  No GPU, no library: a program of its own so that it can
// also be built with -fsanitize=address,undefined.
//   vp8_seg_host <width> <height> <quality> <translucent 0|1> <b_pred 0|1> <adaptive 0|1> <loop filter 0|1> <segments 0|1>
//                <planes.bin> <out.webp> [what a decoder shows.bin]
// It prints one line: "vp8 seg ok <bytes> on <0|1> qi <4> prob <3> level <level>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fl_vp8_ap_core.h"
#include "fl_vp8_i4_core.h"
#include "fl_vp8_lf_core.h"
#include "fl_vp8_seg_core.h"

using namespace fl;

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

template <bool I4, bool AP, bool LF> static int run(Vp8Pic &p, uint32_t w, uint32_t h, uint32_t qi, bool alpha, const std::vector<uint8_t> &planes, char **argv, int argc)
{
    const uint32_t mbs = p.mbw * p.mbh, nparts = vp8_partitions(p.mbh);
    if (I4) analyse_i4(p); else analyse_i16(p);
    p.q = vp8_quant(qi); // (the picture's again: the loop filter's base level comes from qi)

    uint32_t level = 0;
    std::vector<uint8_t> copy;
    if (LF) {
        const uint32_t base = vp8_lf_base_of(qi, -1);
        uint64_t D[kVp8LfCandidates] = {0, 0, 0, 0};
        if (base)
            for (uint32_t k = 0; k < kVp8LfCandidates; ++k) D[k] = candidate_cost<I4>(p, vp8_lf_candidate(base, k), copy);
        level = vp8_lf_choice(base, D);
    }
    candidate_cost<I4>(p, level, copy); // what a decoder will show

    std::vector<uint8_t> tab(kVp8CoefProbs);
    if (AP) {
        std::vector<uint32_t> cnt(kVp8CountWords, 0);
        Vp8Count sink{p.prob, cnt.data()};
        for (uint32_t k = 0; k < mbs * kVp8MbBlocks; ++k) vp8_ap_count_item<I4>(sink, p, k);
        for (uint32_t i = 0; i < kVp8CoefProbs; ++i) tab[i] = vp8_ap_decide(i, cnt[i], cnt[kVp8CoefProbs + i]);
        p.prob = tab.data();
    }

    uint32_t size[9] = {0};
    for (uint32_t k = 0; k <= nparts; ++k) {
        Vp8Bool bw;
        code<I4, AP, LF>(bw, p, qi, k, nparts, level);
        size[k] = bw.pos;
    }
    const Vp8Layout L = vp8_layout(w, h, alpha, nparts, size);
    const uint64_t bound = p.seg ? vp8_seg_max_out_bytes(w, h, I4, AP)
                                 : AP ? (I4 ? vp8_i4_ap_max_out_bytes(w, h) : vp8_ap_max_out_bytes(w, h)) : (I4 ? vp8_i4_max_out_bytes(w, h) : vp8_max_out_bytes(w, h));
    if (L.total > bound || size[0] > (p.seg ? vp8_seg_part0_max_bytes(mbs, I4, AP) : bound)) { std::fprintf(stderr, "vp8_seg_host: the file exceeds its worst case\n"); return 1; }
    std::vector<uint8_t> file(L.total);
    vp8_put_framing(file.data(), L, w, h, alpha, nparts, size);
    if (alpha) {
        const uint8_t *a = planes.data() + (size_t)w * h + 2ull * p.cw * p.ch;
        for (size_t i = 0; i < (size_t)w * h; ++i) file[L.alph + 9u + i] = a[i];
    }
    for (uint32_t k = 0; k <= nparts; ++k) {
        Vp8Bool bw;
        bw.buf = file.data() + L.part[k];
        code<I4, AP, LF>(bw, p, qi, k, nparts, level);
        if (bw.pos != size[k]) { std::fprintf(stderr, "vp8_seg_host: partition %u changed its size\n", k); return 1; }
    }
    if (!write_file(argv[10], file.data(), file.size())) { std::fprintf(stderr, "vp8_seg_host: cannot write the file\n"); return 1; }
    if (argc > 11) {
        // what a decoder shows, cropped to the picture: Y (w x h), U, V (cw x ch)
        std::vector<uint8_t> out;
        const uint8_t *rec = copy.data();
        const size_t rys = (size_t)p.mbw * 16, rcs = (size_t)p.mbw * 8, rysz = rys * p.mbh * 16, rcsz = rcs * p.mbh * 8;
        for (uint32_t y = 0; y < h; ++y) out.insert(out.end(), rec + y * rys, rec + y * rys + w);
        for (int pl = 0; pl < 2; ++pl)
            for (uint32_t y = 0; y < p.ch; ++y) out.insert(out.end(), rec + rysz + pl * rcsz + y * rcs, rec + rysz + pl * rcsz + y * rcs + p.cw);
        if (!write_file(argv[11], out.data(), out.size())) return 1;
    }
    Vp8SegRec r{{(uint8_t)qi, (uint8_t)qi, (uint8_t)qi, (uint8_t)qi}, {255, 255, 255}, 0};
    if (p.seg) r = *p.seg;
    std::printf("vp8 seg ok %u on %u qi %u %u %u %u prob %u %u %u level %u\n", L.total, (unsigned)r.on, (unsigned)r.qi[0], (unsigned)r.qi[1], (unsigned)r.qi[2],
                (unsigned)r.qi[3], (unsigned)r.prob[0], (unsigned)r.prob[1], (unsigned)r.prob[2], level);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 11) { std::fprintf(stderr, "usage: vp8_seg_host <width> <height> <quality> <translucent> <b_pred> <adaptive> <loop filter> <segments> <planes.bin> <out.webp> [shown.bin]\n"); return 2; }
    const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]), quality = (uint32_t)std::atoi(argv[3]);
    const bool alpha = std::atoi(argv[4]) != 0, i4 = std::atoi(argv[5]) != 0, adapt = std::atoi(argv[6]) != 0, lf = std::atoi(argv[7]) != 0, segments = std::atoi(argv[8]) != 0;
    if (!vp8_seg_fits(w, h, i4, true) || quality < 1 || quality > 99) { std::fprintf(stderr, "vp8_seg_host: outside the coder's limits\n"); return 2; }
    Vp8Pic p;
    vp8_pic_dims(p, w, h);
    std::vector<uint8_t> planes(2ull * w * h + 2ull * p.cw * p.ch);
    if (!read_file(argv[9], planes)) { std::fprintf(stderr, "vp8_seg_host: cannot read the planes\n"); return 1; }
    const uint32_t mbs = p.mbw * p.mbh, qi = vp8_quality_index(quality);
    std::vector<uint8_t> rec(vp8_rec_bytes(p.mbw, p.mbh));
    std::vector<int16_t> lev((size_t)mbs * kVp8MbLevels);
    std::vector<uint32_t> info(mbs), bm(2 * (size_t)mbs);
    p.src = planes.data(); p.rec = rec.data(); p.lev = lev.data(); p.info = info.data(); p.bm = i4 ? bm.data() : nullptr;
    p.q = vp8_quant(qi);

    // the segment rule: the bins of the macroblocks, their histogram, the classes and the record
    Vp8SegRec srec;
    std::vector<uint8_t> map(mbs);
    if (segments) {
        uint32_t hist[kVp8SegBins];
        uint8_t cls[kVp8SegBins];
        vp8_seg_bins(planes.data(), w, h, map.data(), hist);
        vp8_seg_classify(hist, qi, srec, cls);
        for (uint32_t mb = 0; mb < mbs; ++mb) map[mb] = cls[map[mb]];
        p.seg = &srec; p.segmap = map.data();
    }
    if (i4) {
        if (adapt) return lf ? run<true, true, true>(p, w, h, qi, alpha, planes, argv, argc) : run<true, true, false>(p, w, h, qi, alpha, planes, argv, argc);
        return lf ? run<true, false, true>(p, w, h, qi, alpha, planes, argv, argc) : run<true, false, false>(p, w, h, qi, alpha, planes, argv, argc);
    }
    if (adapt) return lf ? run<false, true, true>(p, w, h, qi, alpha, planes, argv, argc) : run<false, true, false>(p, w, h, qi, alpha, planes, argv, argc);
    return lf ? run<false, false, true>(p, w, h, qi, alpha, planes, argv, argc) : run<false, false, false>(p, w, h, qi, alpha, planes, argv, argc);
}
