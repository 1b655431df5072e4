// vp8_src_fuzz.cpp -- the host half of the lossy WebP decode front end (csrc/fl_vp8src.cpp) under seeded mutations.
// A stand-alone program: tests/test_vp8_source_host.py compiles it together with fl_vp8src.cpp and fl_webpsrc.cpp with
// -fsanitize=address,undefined and runs it on the CPU.  usage: vp8_src_fuzz <mutations per file> <file>...
// For every file: the intact file must decode to a blob of the size the deep parse announces; then N mutants (byte overwrites,
// bit flips, truncations with the RIFF and chunk sizes repaired, edits of the frame tag and the partition sizes) go through
// vp8_parse_info (shallow and deep) and vp8_decode_levels, whose buffer has exactly the capacity the header asks for (a write
// past it is a heap overflow the sanitizer reports).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fl_vp8src.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static void put32(std::vector<uint8_t> &d, size_t at, uint32_t v)
{
    if (at + 4 <= d.size()) { d[at] = (uint8_t)v; d[at + 1] = (uint8_t)(v >> 8); d[at + 2] = (uint8_t)(v >> 16); d[at + 3] = (uint8_t)(v >> 24); }
}

// offset of the "VP8 " chunk header, 0 if there is none where the walk gets to
static size_t vp8_chunk(const std::vector<uint8_t> &d)
{
    for (size_t pos = 12; pos + 8 <= d.size();) {
        if (!memcmp(d.data() + pos, "VP8 ", 4)) return pos;
        const size_t len = (size_t)d[pos + 4] | (size_t)d[pos + 5] << 8 | (size_t)d[pos + 6] << 16 | (size_t)d[pos + 7] << 24;
        if (len > d.size()) return 0;
        pos += 8 + len + (len & 1u);
    }
    return 0;
}

// after a truncation: the RIFF size and the VP8 chunk's size say what is left, so that the stream itself ends early
static void repair_sizes(std::vector<uint8_t> &d)
{
    if (d.size() & 1u) d.push_back(0);
    if (d.size() < 20) return;
    put32(d, 4, (uint32_t)d.size() - 8u);
    const size_t at = vp8_chunk(d);
    if (at) put32(d, at + 4, (uint32_t)(d.size() - at - 8u));
}

// 0 = decoded with the announced blob size, 1 = refused with a clean error code, 2 = a wrong result
static int run(const std::vector<uint8_t> &d)
{
    std::vector<uint8_t> file(d); // an exact-size copy: a read past the file's end is a heap overflow too
    fl::Vp8Info shallow, info;
    if (fl::vp8_parse_info(file.data(), file.size(), shallow, false) != 0) return 1;
    const int drc = fl::vp8_parse_info(file.data(), file.size(), info, true);
    if (!shallow.supported) return 1;
    const size_t cap = fl::vp8_blob_capacity(shallow);
    if (cap > ((size_t)256 << 20)) return 1; // (the fuzzer keeps its heap small)
    uint8_t *blob = static_cast<uint8_t *>(aligned_alloc(16, (cap + 15u) & ~(size_t)15u));
    fl::Vp8BlobHeader H;
    const int rc = fl::vp8_decode_levels(file.data(), file.size(), blob, cap, &H);
    int result = 1;
    if (rc == 0) {
        result = 0;
        if (drc != 0 || H.magic != fl::kVp8BlobMagic || H.width != shallow.width || H.height != shallow.height || H.total_bytes > cap ||
            H.total_bytes != info.blob_bytes || H.lev_off + (size_t)H.nlevels * 2u > H.alpha_off || H.alpha_off > H.total_bytes) result = 2;
        else {
            const fl::Vp8MbRecord *r = reinterpret_cast<const fl::Vp8MbRecord *>(blob + H.rec_off);
            uint64_t sum = 0;
            for (size_t i = 0; i < (size_t)H.mbw * H.mbh; ++i) {
                if (r[i].lev != sum) result = 2;
                for (int b = 0; b < 25; ++b) { if (r[i].cnt[b] > 16) result = 2; sum += r[i].cnt[b]; }
            }
            if (sum != H.nlevels) result = 2;
        }
    } else if (rc != fl::kVp8Parse && rc != fl::kVp8Unsupported && rc != fl::kVp8Small) result = 2;
    // the deep parse reads what the decode reads -- but of a compressed ALPH chunk only the transform headers, not the plane's own stream
    else if (!shallow.alpha_compression && (rc == fl::kVp8Parse) != (drc != 0)) result = 2;
    else if (shallow.alpha_compression && drc != 0 && rc == 0) result = 2;
    free(blob);
    return result;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s <mutations> <file>...\n", argv[0]); return 2; }
    const int n = atoi(argv[1]);
    for (int a = 2; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> orig;
        uint8_t buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) orig.insert(orig.end(), buf, buf + k);
        fclose(f);
        const bool intact = run(orig) == 0;
        const size_t frame = vp8_chunk(orig) + 8u;
        int refused = 0, wrong = 0;
        rng_state = 0x9e3779b97f4a7c15ull + (uint64_t)a;
        for (int m = 0; m < n; ++m) {
            std::vector<uint8_t> d(orig);
            const uint32_t kind = rnd() % 10u, edits = 1u + rnd() % 3u;
            for (uint32_t e = 0; e < edits; ++e) {
                const size_t at = rnd() % d.size();
                if (kind < 3) d[at] = (uint8_t)rnd();
                else if (kind < 6) d[at] ^= (uint8_t)(1u << (rnd() % 8u));
                else if (kind == 6) { d.resize(at ? at : 1); repair_sizes(d); break; }
                else if (kind == 7) put32(d, (rnd() & 1u) ? 4 : frame - 4u, (rnd() & 1u) ? rnd() : (uint32_t)d.size() - (rnd() % 40u)); // the length fields
                else if (kind == 8) { const size_t k = frame + rnd() % 24u; if (k < d.size()) d[k] = (uint8_t)rnd(); } // frame tag, sizes, the first header bits
                else d[at] = (uint8_t)(rnd() & 1u ? 0xffu : 0u);
            }
            const int r = run(d);
            refused += r == 1;
            wrong += r == 2;
        }
        printf("file %s intact=%s mutants=%d refused=%d wrong=%d\n", argv[a], intact ? "ok" : "FAILED", n, refused, wrong);
        if (!intact || wrong) return 1;
    }
    return 0;
}
