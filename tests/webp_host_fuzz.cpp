// webp_host_fuzz.cpp -- the host half of the lossless WebP decode front end (csrc/fl_webpsrc.cpp) under seeded mutations.
// A stand-alone program: tests/test_webp_source_host.py compiles it together with fl_webpsrc.cpp with
// -fsanitize=address,undefined and runs it on the CPU.  usage: webp_host_fuzz <mutations per file> <file>...
// For every file: the intact file must decode to a blob of the pixel count its header announces; then N mutants (byte
// overwrites, bit flips, truncations with the RIFF and chunk sizes repaired, edits of the length fields themselves) go through
// webp_parse_info (shallow and deep) and webp_decode_residuals, whose buffer has exactly the capacity the header asks for
// (a write past it is a heap overflow the sanitizer reports).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fl_webpsrc.h"

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

// after a truncation: the RIFF size and the (single) VP8L chunk's size say what is left, so that the stream itself ends early
static void repair_sizes(std::vector<uint8_t> &d)
{
    if (d.size() & 1u) d.push_back(0);
    if (d.size() < 20) return;
    put32(d, 4, (uint32_t)d.size() - 8u);
    if (!memcmp(d.data() + 12, "VP8L", 4)) put32(d, 16, (uint32_t)d.size() - 20u);
}

// 0 = decoded with the right pixel count, 1 = refused with a clean error code, 2 = a wrong result
static int run(const std::vector<uint8_t> &d)
{
    std::vector<uint8_t> file(d); // an exact-size copy: a read past the file's end is a heap overflow too
    fl::WebpInfo shallow, info;
    if (fl::webp_parse_info(file.data(), file.size(), shallow, false) != 0) return 1;
    const int drc = fl::webp_parse_info(file.data(), file.size(), info, true);
    if (!shallow.supported) return 1;
    const size_t cap = fl::webp_blob_capacity(shallow, file.size());
    if (cap > ((size_t)256 << 20)) return 1; // (the fuzzer keeps its heap small)
    uint8_t *blob = static_cast<uint8_t *>(aligned_alloc(16, (cap + 15u) & ~(size_t)15u));
    fl::WebpBlobHeader H;
    const int rc = fl::webp_decode_residuals(file.data(), file.size(), blob, cap, &H);
    int result = 1;
    if (rc == 0) {
        result = 0;
        if (drc != 0 || H.magic != fl::kWebpMagic || H.width != shallow.width || H.height != shallow.height || H.total_bytes > cap ||
            (size_t)H.res_off + (size_t)H.xsize * H.height * 4u != H.total_bytes || H.ntransforms > 4) result = 2;
    } else if (rc != fl::kWebpParse && rc != fl::kWebpUnsupported && rc != fl::kWebpSmall) result = 2;
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
        int refused = 0, wrong = 0;
        rng_state = 0x9e3779b97f4a7c15ull + (uint64_t)a;
        for (int m = 0; m < n; ++m) {
            std::vector<uint8_t> d(orig);
            const uint32_t kind = rnd() % 9u, edits = 1u + rnd() % 3u;
            for (uint32_t e = 0; e < edits; ++e) {
                const size_t at = rnd() % d.size();
                if (kind < 3) d[at] = (uint8_t)rnd();
                else if (kind < 6) d[at] ^= (uint8_t)(1u << (rnd() % 8u));
                else if (kind == 6) { d.resize(at ? at : 1); repair_sizes(d); break; }
                else if (kind == 7) put32(d, (rnd() & 1u) ? 4 : 16, (rnd() & 1u) ? rnd() : (uint32_t)d.size() - (rnd() % 40u)); // the length fields
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
