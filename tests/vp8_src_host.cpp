// vp8_src_host.cpp -- the host twin of the lossy WebP decoder: csrc/fl_vp8src.cpp's levels through the functions of
// csrc/fl_vp8dec_core.h, which the kernels of fl_vp8dec.hip spread over lanes, here in plain loops on the CPU: macroblocks in
// raster order, the steps of each one after the other.  (The ALPH filters 1 and 2 are prefix sums on the device; here they are
// the sums' definition.)
//   vp8_src_host <file.webp> <out> [<green>]   writes to <out>: the padded Y | U | V planes before the loop filter, the same
//                                     after it, and the Rgb8 / Rgba8 pixels; prints "w h channels mbw mbh blob_bytes".  <green>: for a
//                                     file with a compressed ALPH chunk, the green channel of the lossless blob behind the levels with
//                                     its transforms inverted (w x h bytes; the caller's numpy inverse of tests/vp8l_write.py) -- the
//                                     device runs the lossless decoder's kernels there.  Without it such a file's alpha reads 255.
// Exit status 3 = kVp8Parse, 4 = kVp8Unsupported, 5 = the blob did not fit its announced capacity.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fl_vp8dec_core.h"

using namespace fl;

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s <file.webp> <out> [<green>]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + k);
    fclose(f);
    Vp8Info info;
    int rc = vp8_parse_info(file.data(), file.size(), info, true);
    if (rc) return rc == kVp8Parse ? 3 : 4;
    if (!info.supported) return 4;
    const size_t cap = vp8_blob_capacity(info);
    uint8_t *blob = static_cast<uint8_t *>(aligned_alloc(16, (cap + 15u) & ~(size_t)15u));
    Vp8BlobHeader H;
    rc = vp8_decode_levels(file.data(), file.size(), blob, cap, &H);
    if (rc) return rc == kVp8Parse ? 3 : rc == kVp8Unsupported ? 4 : 5;
    if (H.total_bytes != info.blob_bytes || H.total_bytes > cap) return 5;

    std::vector<uint8_t> planes(vp8_rec_bytes(H.mbw, H.mbh));
    Vp8DecPic p;
    vp8d_pic(p, blob, planes.data());
    for (uint32_t mby = 0; mby < p.mbh; ++mby)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx) {
            const Vp8MbRecord &r = p.recs[(size_t)mby * p.mbw + mbx];
            Vp8DecWork w;
            for (uint32_t k = 0; k < 4; ++k) vp8d_prepare(p, r, w, mbx, mby, k);
            for (uint32_t b = 0; b < 24; ++b) vp8d_residual(p, r, w, b);
            for (uint32_t s = 0; s < kVp8dSubSteps; ++s)
                for (uint32_t lane = 0; lane < kVp8dLanes; ++lane) vp8d_reconstruct(p, r, w, mbx, mby, s, lane);
        }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(planes.data(), 1, planes.size(), o);
    for (uint32_t mby = 0; mby < p.mbh; ++mby)
        for (uint32_t mbx = 0; mbx < p.mbw; ++mbx)
            for (uint32_t s = 0; s < kVp8dFilterSteps; ++s)
                for (uint32_t lane = 0; lane < kVp8dFilterLanes; ++lane) vp8d_filter(p, p.recs[(size_t)mby * p.mbw + mbx], mbx, mby, s, lane);
    fwrite(planes.data(), 1, planes.size(), o);

    const uint32_t w = H.width, h = H.height;
    std::vector<uint8_t> alpha;
    std::vector<uint8_t> green;
    if (H.alpha == 2 && argc == 4) {
        FILE *g = fopen(argv[3], "rb");
        if (!g) return 2;
        green.resize((size_t)w * h);
        if (fread(green.data(), 1, green.size(), g) != green.size()) return 2;
        fclose(g);
    }
    const bool have_alpha = H.alpha == 1 || !green.empty();
    if (have_alpha) {
        const uint8_t *in = H.alpha == 1 ? blob + H.alpha_off : green.data();
        alpha.resize((size_t)w * h);
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t at = (size_t)y * w + x;
                const int left = x ? alpha[at - 1] : y ? alpha[at - w] : 0;
                if (H.alpha_filter == 0) alpha[at] = in[at];
                else if (H.alpha_filter == 1) alpha[at] = (uint8_t)(in[at] + left);
                else if (H.alpha_filter == 2) alpha[at] = (uint8_t)(in[at] + (y ? alpha[at - w] : left));
                else alpha[at] = vp8d_alpha_gradient(in[at], alpha.data(), w, x, y);
            }
    }
    std::vector<uint8_t> px((size_t)w * h * H.channels);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) vp8d_pixel(p, have_alpha ? alpha.data() : nullptr, w, h, H.channels, x, y, px.data() + ((size_t)y * w + x) * H.channels);
    fwrite(px.data(), 1, px.size(), o);
    fclose(o);
    printf("%u %u %u %u %u %u\n", w, h, H.channels, H.mbw, H.mbh, H.total_bytes);
    free(blob);
    return 0;
}
