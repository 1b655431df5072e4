// png_adam7_fuzz.cpp -- the Adam7 side of the host half of the PNG decode front end (csrc/fl_pngsrc.cpp with adam7 = true,
// csrc/fl_png_adam7.h) under seeded mutations.  A stand-alone program: tests/test_png_adam7_host.py compiles it together with
// fl_pngsrc.cpp with -fsanitize=address,undefined and runs it on the CPU.  usage: png_adam7_fuzz <mutations per file> <file>...
// For every file: the intact file must decode and its pass table must add up; then N mutants (byte overwrites, bit flips,
// truncations, CRC-repaired damage so that IHDR -- the sizes the passes follow from -- and the inflate itself see bad data) go
// through png_parse_info and png_decode_scanlines, whose buffers are sized exactly (a write past the size the passes imply, or a
// filter byte looked for past it, is a heap overflow the sanitizer reports).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fl_pngsrc.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static uint32_t crc_of(const uint8_t *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
    }
    return ~c;
}

// recomputes the CRC of every chunk, so that damage inside a chunk reaches the code behind the CRC check
static void repair_crcs(std::vector<uint8_t> &d)
{
    size_t pos = 8;
    while (pos + 12 <= d.size()) {
        const uint32_t len = (uint32_t)d[pos] << 24 | (uint32_t)d[pos + 1] << 16 | (uint32_t)d[pos + 2] << 8 | d[pos + 3];
        if (len > d.size() - pos - 12) break;
        const uint32_t c = crc_of(d.data() + pos + 4, (size_t)len + 4);
        uint8_t *q = d.data() + pos + 8 + len;
        q[0] = (uint8_t)(c >> 24); q[1] = (uint8_t)(c >> 16); q[2] = (uint8_t)(c >> 8); q[3] = (uint8_t)c;
        pos += 12 + (size_t)len;
    }
}

// the passes of a supported interlaced picture lie back to back and end where the stream ends: -1 if they do not
static int passes_add_up(const fl::PngInfo &info)
{
    uint64_t scan = 0, rows = 0;
    for (uint32_t p = 0; p < fl::kAdam7Passes; ++p) {
        const fl::Adam7Pass P = fl::adam7_pass(info.width, info.height, info.pixel_bits, p);
        if (P.scan_off != scan || P.rows_off != rows) return -1;
        if (!P.w || !P.h) continue;
        if (P.row_bytes != ((uint64_t)P.w * info.pixel_bits + 7u) / 8u) return -1;
        scan += (uint64_t)P.h * (1u + P.row_bytes);
        rows += (uint64_t)P.h * P.row_bytes;
    }
    return scan == fl::png_scan_bytes(info) && rows == fl::adam7_rows_bytes(info.width, info.height, info.pixel_bits) ? 0 : -1;
}

// 0 = decoded, 1 = refused, -1 = the pass table contradicts itself; the scanline buffer has exactly the size the header implies
static int run(const std::vector<uint8_t> &d)
{
    // an exact-size copy: a read past the file's end is a heap overflow too
    std::vector<uint8_t> file(d);
    fl::PngInfo info;
    if (fl::png_parse_info(file.data(), file.size(), info, true, true) != 0) return 1;
    if (!info.supported) return 1;
    if (info.interlaced && passes_add_up(info) != 0) return -1;
    const size_t want = fl::png_scan_bytes(info);
    if (want > ((size_t)64 << 20)) return 1; // (png_parse_info bounds it by 1032 x the IDAT bytes; the fuzzer keeps its heap small)
    std::vector<uint8_t> scan(want);
    fl::PngBlobHeader hdr;
    if (fl::png_decode_scanlines(file.data(), file.size(), scan.data(), scan.size(), &hdr, true) != 0) return 1;
    if (hdr.interlaced != info.interlaced || hdr.total_bytes != sizeof(fl::PngBlobHeader) + want || (hdr.interlaced && hdr.direct)) return -1;
    return 0;
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
        int refused = 0, broken = 0;
        rng_state = 0x9e3779b97f4a7c15ull + (uint64_t)a;
        for (int m = 0; m < n; ++m) {
            std::vector<uint8_t> d(orig);
            const uint32_t kind = rnd() % 8u, edits = 1u + rnd() % 3u;
            for (uint32_t e = 0; e < edits; ++e) {
                // every fourth mutant aims at IHDR's width, height, depth and colour type: the passes' sizes follow from them
                const size_t at = (m % 4 == 3 && d.size() > 26) ? 16 + rnd() % 10u : rnd() % d.size();
                if (kind < 3) d[at] = (uint8_t)rnd();
                else if (kind < 6) d[at] ^= (uint8_t)(1u << (rnd() % 8u));
                else if (kind == 6) { d.resize(at ? at : 1); break; }
                else d[at] = (uint8_t)(rnd() & 1u ? 0xffu : 0u);
            }
            if (m & 1) repair_crcs(d);
            const int r = run(d);
            refused += r == 1;
            broken += r < 0;
        }
        printf("file %s intact=%s mutants=%d refused=%d broken=%d\n", argv[a], intact ? "ok" : "FAILED", n, refused, broken);
        if (!intact || broken) return 1;
    }
    return 0;
}
