// The host twin of the lossy WebP encoder's I4 variant (FLGPU_FE_WEBP_LOSSY_I4): the functions of fanlin-rs_amd/csrc/fl_vp8_core.h
// and fl_vp8_i4_core.h -- the ones the kernels of fl_vp8.hip call -- run here in plain loops, from the planes of FLGPU_FE_WEBP420
// (Y | U | V | A) to the finished file.  No GPU, no library: it is a program of its own so that it can also be built with
// -fsanitize=address,undefined.
//   vp8_i4_host <width> <height> <quality> <translucent 0|1> <planes.bin> <out.webp> [reconstruction.bin [modes.bin]]
// modes.bin: per macroblock 17 bytes, 1 if it is B_PRED and its sixteen sub-block modes (fl_vp8_dtables.h's numbers; 0 if it is not).
#include <cstdio>
#include <cstdlib>
#include <vector>

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

int main(int argc, char **argv)
{
    if (argc < 7) { std::fprintf(stderr, "usage: vp8_i4_host <width> <height> <quality> <translucent> <planes.bin> <out.webp> [reconstruction.bin [modes.bin]]\n"); return 2; }
    const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]), quality = (uint32_t)std::atoi(argv[3]);
    const bool alpha = std::atoi(argv[4]) != 0;
    if (!vp8_i4_fits(w, h) || quality < 1 || quality > 99) { std::fprintf(stderr, "vp8_i4_host: outside the coder's limits\n"); return 2; }
    Vp8Pic p;
    vp8_pic_dims(p, w, h);
    std::vector<uint8_t> planes(2ull * w * h + 2ull * p.cw * p.ch);
    if (!read_file(argv[5], planes)) { std::fprintf(stderr, "vp8_i4_host: cannot read the planes\n"); return 1; }
    const uint32_t mbs = p.mbw * p.mbh, qi = vp8_quality_index(quality), nparts = vp8_partitions(p.mbh);
    std::vector<uint8_t> rec(vp8_rec_bytes(p.mbw, p.mbh));
    std::vector<int16_t> lev((size_t)mbs * kVp8MbLevels);
    std::vector<uint32_t> info(mbs), bm(2 * (size_t)mbs);
    p.src = planes.data(); p.rec = rec.data(); p.lev = lev.data(); p.info = info.data(); p.bm = bm.data();
    p.q = vp8_quant(qi);

    // predict, transform, quantise, reconstruct: macroblocks in raster order, every phase over all of its items
    uint32_t skipped = 0, bpred = 0;
    for (uint32_t mby = 0; mby < p.mbh; ++mby)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) {
            Vp8Mb m;
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
            skipped += vp8_coded<true>(p, (size_t)mby * p.mbw + mbx) == 0;
            bpred += i4;
        }

    // sizes first (the coder only counts), then every partition at its place in the file
    uint32_t size[9] = {0};
    for (uint32_t k = 0; k <= nparts; ++k) {
        Vp8Bool bw;
        if (k == 0) vp8_put_first_partition<true>(bw, p, qi, nparts);
        else vp8_put_token_partition<true>(bw, p, k - 1, nparts);
        size[k] = bw.pos;
    }
    const Vp8Layout L = vp8_layout(w, h, alpha, nparts, size);
    if (L.total > vp8_i4_max_out_bytes(w, h)) { std::fprintf(stderr, "vp8_i4_host: the file exceeds its worst case\n"); return 1; }
    std::vector<uint8_t> file(L.total);
    vp8_put_framing(file.data(), L, w, h, alpha, nparts, size);
    if (alpha) {
        const uint8_t *a = planes.data() + (size_t)w * h + 2ull * p.cw * p.ch;
        for (size_t i = 0; i < (size_t)w * h; ++i) file[L.alph + 9u + i] = a[i];
    }
    for (uint32_t k = 0; k <= nparts; ++k) {
        Vp8Bool bw;
        bw.buf = file.data() + L.part[k];
        if (k == 0) vp8_put_first_partition<true>(bw, p, qi, nparts);
        else vp8_put_token_partition<true>(bw, p, k - 1, nparts);
        if (bw.pos != size[k]) { std::fprintf(stderr, "vp8_i4_host: partition %u changed its size\n", k); return 1; }
    }
    if (!write_file(argv[6], file.data(), file.size())) { std::fprintf(stderr, "vp8_i4_host: cannot write the file\n"); return 1; }
    if (argc > 7) {
        // the reconstruction cropped to the picture: Y (w x h), U, V (cw x ch)
        std::vector<uint8_t> out;
        const size_t rys = (size_t)p.mbw * 16, rcs = (size_t)p.mbw * 8, rysz = rys * p.mbh * 16, rcsz = rcs * p.mbh * 8;
        for (uint32_t y = 0; y < h; ++y) out.insert(out.end(), rec.begin() + y * rys, rec.begin() + y * rys + w);
        for (int pl = 0; pl < 2; ++pl)
            for (uint32_t y = 0; y < p.ch; ++y) out.insert(out.end(), rec.begin() + rysz + pl * rcsz + y * rcs, rec.begin() + rysz + pl * rcsz + y * rcs + p.cw);
        if (!write_file(argv[7], out.data(), out.size())) return 1;
    }
    if (argc > 8) {
        std::vector<uint8_t> out;
        for (uint32_t mb = 0; mb < mbs; ++mb) {
            const bool i4 = vp8_is_i4(p, mb);
            out.push_back(i4);
            for (uint32_t b = 0; b < 16; ++b) out.push_back(i4 ? (uint8_t)vp8_bm_nibble(p, mb, b) : 0);
        }
        if (!write_file(argv[8], out.data(), out.size())) return 1;
    }
    std::printf("vp8 i4 ok %u bytes, %u of %u macroblocks skipped, %u B_PRED\n", L.total, skipped, mbs, bpred);
    return 0;
}
