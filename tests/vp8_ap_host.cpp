// The host twin of the lossy WebP encoder's adaptive-probability variants (FLGPU_FE_WEBP_LOSSY_AP, FLGPU_FE_WEBP_LOSSY_I4_AP): the
// functions of fanlin-rs_amd/csrc/fl_vp8_core.h, fl_vp8_i4_core.h and fl_vp8_ap_core.h -- the ones the kernels of fl_vp8.hip call --
// run here in plain loops, from the planes of FLGPU_FE_WEBP420 (Y | U | V | A) to the finished file: the analysis of the front end
// the variant stands beside, the counting walk over every (macroblock, block) item, the rule per table entry, the coder with the
// picture's table.  No GPU, no library: it is a program of its own so that it can also be built with -fsanitize=address,undefined.
//   vp8_ap_host <width> <height> <quality> <translucent 0|1> <b_pred 0|1> <planes.bin> <out.webp> [reconstruction.bin [stats.bin]]
// stats.bin: the 1056 zero counts and the 1056 one counts (little-endian 32-bit words), then the picture's 1056 probabilities.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fl_vp8_ap_core.h"
#include "fl_vp8_i4_core.h"

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

template <bool I4> static void code(Vp8Bool &bw, const Vp8Pic &p, uint32_t qi, uint32_t part, uint32_t nparts)
{
    if (part == 0) vp8_put_first_partition<I4, true>(bw, p, qi, nparts);
    else vp8_put_token_partition<I4>(bw, p, part - 1, nparts);
}

template <bool I4> static int run(Vp8Pic &p, uint32_t w, uint32_t h, uint32_t qi, bool alpha, const std::vector<uint8_t> &planes, char **argv, int argc)
{
    const uint32_t mbs = p.mbw * p.mbh, nparts = vp8_partitions(p.mbh);
    if (I4) analyse_i4(p); else analyse_i16(p);

    // the statistics: every (macroblock, block) item on its own, as the kernel's threads take them; then the rule per entry
    std::vector<uint32_t> cnt(kVp8CountWords, 0);
    Vp8Count sink{p.prob, cnt.data()};
    for (uint32_t k = 0; k < mbs * kVp8MbBlocks; ++k) vp8_ap_count_item<I4>(sink, p, k);
    std::vector<uint8_t> tab(kVp8CoefProbs);
    for (uint32_t i = 0; i < kVp8CoefProbs; ++i) tab[i] = vp8_ap_decide(i, cnt[i], cnt[kVp8CoefProbs + i]);
    p.prob = tab.data();

    // sizes first (the coder only counts), then every partition at its place in the file
    uint32_t size[9] = {0};
    for (uint32_t k = 0; k <= nparts; ++k) {
        Vp8Bool bw;
        code<I4>(bw, p, qi, k, nparts);
        size[k] = bw.pos;
    }
    const Vp8Layout L = vp8_layout(w, h, alpha, nparts, size);
    if (L.total > (I4 ? vp8_i4_ap_max_out_bytes(w, h) : vp8_ap_max_out_bytes(w, h))) { std::fprintf(stderr, "vp8_ap_host: the file exceeds its worst case\n"); return 1; }
    std::vector<uint8_t> file(L.total);
    vp8_put_framing(file.data(), L, w, h, alpha, nparts, size);
    if (alpha) {
        const uint8_t *a = planes.data() + (size_t)w * h + 2ull * p.cw * p.ch;
        for (size_t i = 0; i < (size_t)w * h; ++i) file[L.alph + 9u + i] = a[i];
    }
    for (uint32_t k = 0; k <= nparts; ++k) {
        Vp8Bool bw;
        bw.buf = file.data() + L.part[k];
        code<I4>(bw, p, qi, k, nparts);
        if (bw.pos != size[k]) { std::fprintf(stderr, "vp8_ap_host: partition %u changed its size\n", k); return 1; }
    }
    if (!write_file(argv[7], file.data(), file.size())) { std::fprintf(stderr, "vp8_ap_host: cannot write the file\n"); return 1; }
    if (argc > 8) {
        // the reconstruction cropped to the picture: Y (w x h), U, V (cw x ch)
        std::vector<uint8_t> out;
        const uint8_t *rec = p.rec;
        const size_t rys = (size_t)p.mbw * 16, rcs = (size_t)p.mbw * 8, rysz = rys * p.mbh * 16, rcsz = rcs * p.mbh * 8;
        for (uint32_t y = 0; y < h; ++y) out.insert(out.end(), rec + y * rys, rec + y * rys + w);
        for (int pl = 0; pl < 2; ++pl)
            for (uint32_t y = 0; y < p.ch; ++y) out.insert(out.end(), rec + rysz + pl * rcsz + y * rcs, rec + rysz + pl * rcsz + y * rcs + p.cw);
        if (!write_file(argv[8], out.data(), out.size())) return 1;
    }
    if (argc > 9) {
        std::vector<uint8_t> out;
        for (uint32_t v : cnt) for (int b = 0; b < 4; ++b) out.push_back((uint8_t)(v >> (8 * b)));
        out.insert(out.end(), tab.begin(), tab.end());
        if (!write_file(argv[9], out.data(), out.size())) return 1;
    }
    uint32_t updates = 0;
    for (uint32_t i = 0; i < kVp8CoefProbs; ++i) updates += tab[i] != kVp8CoefProb[i];
    std::printf("vp8 ap ok %u bytes, %u of 1056 probabilities updated\n", L.total, updates);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 8) { std::fprintf(stderr, "usage: vp8_ap_host <width> <height> <quality> <translucent> <b_pred> <planes.bin> <out.webp> [reconstruction.bin [stats.bin]]\n"); return 2; }
    const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]), quality = (uint32_t)std::atoi(argv[3]);
    const bool alpha = std::atoi(argv[4]) != 0, i4 = std::atoi(argv[5]) != 0;
    if (!(i4 ? vp8_i4_ap_fits(w, h) : vp8_ap_fits(w, h)) || quality < 1 || quality > 99) { std::fprintf(stderr, "vp8_ap_host: outside the coder's limits\n"); return 2; }
    Vp8Pic p;
    vp8_pic_dims(p, w, h);
    std::vector<uint8_t> planes(2ull * w * h + 2ull * p.cw * p.ch);
    if (!read_file(argv[6], planes)) { std::fprintf(stderr, "vp8_ap_host: cannot read the planes\n"); return 1; }
    const uint32_t mbs = p.mbw * p.mbh, qi = vp8_quality_index(quality);
    std::vector<uint8_t> rec(vp8_rec_bytes(p.mbw, p.mbh));
    std::vector<int16_t> lev((size_t)mbs * kVp8MbLevels);
    std::vector<uint32_t> info(mbs), bm(2 * (size_t)mbs);
    p.src = planes.data(); p.rec = rec.data(); p.lev = lev.data(); p.info = info.data(); p.bm = i4 ? bm.data() : nullptr;
    p.q = vp8_quant(qi);
    return i4 ? run<true>(p, w, h, qi, alpha, planes, argv, argc) : run<false>(p, w, h, qi, alpha, planes, argv, argc);
}
