// The host twin of the lossy WebP encoder's loop-filtered variants (FLGPU_FE_WEBP_LOSSY_LF, _I4_LF, _AP_LF, _I4_AP_LF): the functions
// of fanlin-rs_amd/csrc/fl_vp8_core.h, fl_vp8_i4_core.h, fl_vp8_ap_core.h and fl_vp8_lf_core.h -- the ones the kernels of fl_vp8.hip
// call -- run here in plain loops, from the planes of FLGPU_FE_WEBP420 (Y | U | V | A) to the finished file: the analysis of the twin
// front end, per candidate level the decode front end's filter over a copy of the reconstruction (macroblocks in raster order, the
// eight steps of each, the 32 lines of a step) and the squared error over the visible samples, the choice, the coder with the
// level in the frame header.  No GPU, no library: a program of its own so that it can also be built with -fsanitize=address,undefined.
//   vp8_lf_host <width> <height> <quality> <translucent 0|1> <b_pred 0|1> <adaptive 0|1> <base level, -1 = from the quantiser>
//               <planes.bin> <out.webp> [filtered reconstruction.bin]
// It prints one line: "vp8 lf ok <bytes> levels <4> D <4> chosen <level>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fl_vp8_ap_core.h"
#include "fl_vp8_i4_core.h"
#include "fl_vp8_lf_core.h"

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
static void analyse_i16(const Vp8Pic &p)
{
    for (uint32_t mby = 0; mby < p.mbh; ++mby)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) {
            Vp8Mb m;
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

static void analyse_i4(const Vp8Pic &p)
{
    for (uint32_t mby = 0; mby < p.mbh; ++mby)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) {
            Vp8Mb m;
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

template <bool I4, bool AP> static void code(Vp8Bool &bw, const Vp8Pic &p, uint32_t qi, uint32_t part, uint32_t nparts, uint32_t level)
{
    if (part == 0) vp8_put_first_partition<I4, AP, true>(bw, p, qi, nparts, level);
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

template <bool I4, bool AP> static int run(Vp8Pic &p, uint32_t w, uint32_t h, uint32_t qi, bool alpha, int forced, const std::vector<uint8_t> &planes, char **argv, int argc)
{
    const uint32_t mbs = p.mbw * p.mbh, nparts = vp8_partitions(p.mbh);
    if (I4) analyse_i4(p); else analyse_i16(p);

    // the level: four candidates, each filtered and measured on a copy of its own
    const uint32_t base = vp8_lf_base_of(qi, forced);
    uint64_t D[kVp8LfCandidates] = {0, 0, 0, 0};
    std::vector<uint8_t> copy;
    if (base)
        for (uint32_t k = 0; k < kVp8LfCandidates; ++k) D[k] = candidate_cost<I4>(p, vp8_lf_candidate(base, k), copy);
    const uint32_t level = vp8_lf_choice(base, D);
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
        code<I4, AP>(bw, p, qi, k, nparts, level);
        size[k] = bw.pos;
    }
    const Vp8Layout L = vp8_layout(w, h, alpha, nparts, size);
    const uint64_t bound = AP ? (I4 ? vp8_i4_ap_max_out_bytes(w, h) : vp8_ap_max_out_bytes(w, h)) : (I4 ? vp8_i4_max_out_bytes(w, h) : vp8_max_out_bytes(w, h));
    if (L.total > bound) { std::fprintf(stderr, "vp8_lf_host: the file exceeds its worst case\n"); return 1; }
    std::vector<uint8_t> file(L.total);
    vp8_put_framing(file.data(), L, w, h, alpha, nparts, size);
    if (alpha) {
        const uint8_t *a = planes.data() + (size_t)w * h + 2ull * p.cw * p.ch;
        for (size_t i = 0; i < (size_t)w * h; ++i) file[L.alph + 9u + i] = a[i];
    }
    for (uint32_t k = 0; k <= nparts; ++k) {
        Vp8Bool bw;
        bw.buf = file.data() + L.part[k];
        code<I4, AP>(bw, p, qi, k, nparts, level);
        if (bw.pos != size[k]) { std::fprintf(stderr, "vp8_lf_host: partition %u changed its size\n", k); return 1; }
    }
    if (!write_file(argv[9], file.data(), file.size())) { std::fprintf(stderr, "vp8_lf_host: cannot write the file\n"); return 1; }
    if (argc > 10) {
        // the filtered reconstruction cropped to the picture: Y (w x h), U, V (cw x ch)
        std::vector<uint8_t> out;
        const uint8_t *rec = copy.data();
        const size_t rys = (size_t)p.mbw * 16, rcs = (size_t)p.mbw * 8, rysz = rys * p.mbh * 16, rcsz = rcs * p.mbh * 8;
        for (uint32_t y = 0; y < h; ++y) out.insert(out.end(), rec + y * rys, rec + y * rys + w);
        for (int pl = 0; pl < 2; ++pl)
            for (uint32_t y = 0; y < p.ch; ++y) out.insert(out.end(), rec + rysz + pl * rcsz + y * rcs, rec + rysz + pl * rcsz + y * rcs + p.cw);
        if (!write_file(argv[10], out.data(), out.size())) return 1;
    }
    std::printf("vp8 lf ok %u levels %u %u %u %u D %llu %llu %llu %llu chosen %u\n", L.total, vp8_lf_candidate(base, 0), vp8_lf_candidate(base, 1),
                vp8_lf_candidate(base, 2), vp8_lf_candidate(base, 3), (unsigned long long)D[0], (unsigned long long)D[1], (unsigned long long)D[2],
                (unsigned long long)D[3], level);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 10) { std::fprintf(stderr, "usage: vp8_lf_host <width> <height> <quality> <translucent> <b_pred> <adaptive> <base> <planes.bin> <out.webp> [filtered.bin]\n"); return 2; }
    const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]), quality = (uint32_t)std::atoi(argv[3]);
    const bool alpha = std::atoi(argv[4]) != 0, i4 = std::atoi(argv[5]) != 0, adapt = std::atoi(argv[6]) != 0;
    const int forced = std::atoi(argv[7]);
    if (!(i4 ? vp8_i4_ap_fits(w, h) : vp8_ap_fits(w, h)) || quality < 1 || quality > 99 || forced < -1 || forced > 63) { std::fprintf(stderr, "vp8_lf_host: outside the coder's limits\n"); return 2; }
    Vp8Pic p;
    vp8_pic_dims(p, w, h);
    std::vector<uint8_t> planes(2ull * w * h + 2ull * p.cw * p.ch);
    if (!read_file(argv[8], planes)) { std::fprintf(stderr, "vp8_lf_host: cannot read the planes\n"); return 1; }
    const uint32_t mbs = p.mbw * p.mbh, qi = vp8_quality_index(quality);
    std::vector<uint8_t> rec(vp8_rec_bytes(p.mbw, p.mbh));
    std::vector<int16_t> lev((size_t)mbs * kVp8MbLevels);
    std::vector<uint32_t> info(mbs), bm(2 * (size_t)mbs);
    p.src = planes.data(); p.rec = rec.data(); p.lev = lev.data(); p.info = info.data(); p.bm = i4 ? bm.data() : nullptr;
    p.q = vp8_quant(qi);
    if (i4) return adapt ? run<true, true>(p, w, h, qi, alpha, forced, planes, argv, argc) : run<true, false>(p, w, h, qi, alpha, forced, planes, argv, argc);
    return adapt ? run<false, true>(p, w, h, qi, alpha, forced, planes, argv, argc) : run<false, false>(p, w, h, qi, alpha, forced, planes, argv, argc);
}
