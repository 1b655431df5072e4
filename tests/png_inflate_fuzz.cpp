// png_inflate_fuzz.cpp -- the host twin of the PNG inflate kernel (png_inflate_model, csrc/fl_pngsrc.cpp over csrc/fl_inflate_core.h)
// under seeded mutations.  A stand-alone program: tests/test_png_inflate_host.py compiles it together with fl_pngsrc.cpp with
// -fsanitize=address,undefined and runs it on the CPU.  usage: png_inflate_fuzz <mutations per file> <file>...
// The twin runs the kernel's functions over arrays of the kernel's LDS sizes, so an index that would leave an array on the device is a
// report here.  For every file: the intact file must inflate; then N mutants of the IDAT payload (byte overwrites, bit flips, truncations;
// chunk CRCs repaired, so that the damage reaches the inflate).  Whenever the twin says yes, png_decode_scanlines must say yes with
// identical bytes: the device may never accept what the host refuses.  Buffers are sized exactly.
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

// [first, last) of the bytes that are IDAT payload, and the CRCs repaired
struct Span { size_t a, b; };
static std::vector<Span> idat_spans(const std::vector<uint8_t> &d)
{
    std::vector<Span> out;
    size_t pos = 8;
    while (pos + 12 <= d.size()) {
        const uint32_t len = (uint32_t)d[pos] << 24 | (uint32_t)d[pos + 1] << 16 | (uint32_t)d[pos + 2] << 8 | d[pos + 3];
        if (len > d.size() - pos - 12) break;
        if (!memcmp(d.data() + pos + 4, "IDAT", 4) && len) out.push_back({pos + 8, pos + 8 + len});
        pos += 12 + (size_t)len;
    }
    return out;
}
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

// 0 = the twin inflated it (and the host inflate agrees byte for byte), 1 = the twin said no, 2 = the twin accepted what the host refuses or differs
static int run(const std::vector<uint8_t> &d)
{
    std::vector<uint8_t> file(d); // an exact-size copy: a read past the file's end is a heap overflow too
    fl::PngInfo info;
    if (fl::png_parse_info(file.data(), file.size(), info, true, true) != 0) return 1;
    if (!info.supported) return 1;
    const size_t want = fl::png_scan_bytes(info);
    if (want > ((size_t)64 << 20)) return 1;
    std::vector<uint8_t> staged(fl::png_stage_bytes(info));
    fl::PngBlobHeader hdr;
    if (fl::png_stage_compressed(file.data(), file.size(), staged.data(), staged.size(), &hdr, true) != 0) return 1;
    std::vector<uint8_t> scan(want), host(want);
    uint32_t stats[8];
    if (fl::png_inflate_model(staged.data(), staged.size(), scan.data(), scan.size(), stats) != 0) return 1;
    if (fl::png_decode_scanlines(file.data(), file.size(), host.data(), host.size(), nullptr, true) != 0) return 2;
    return scan == host ? 0 : 2;
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
        const std::vector<Span> spans = idat_spans(orig);
        if (spans.empty()) { fprintf(stderr, "%s: no IDAT\n", argv[a]); return 2; }
        int refused = 0, accepted = 0;
        rng_state = 0x9e3779b97f4a7c15ull + (uint64_t)a;
        for (int m = 0; m < n; ++m) {
            std::vector<uint8_t> d(orig);
            const uint32_t kind = rnd() % 8u, edits = 1u + rnd() % 3u;
            for (uint32_t e = 0; e < edits; ++e) {
                const Span &s = spans[rnd() % spans.size()];
                // (half of the edits fall into the first 64 bytes: block headers and code lengths)
                const size_t len = s.b - s.a, at = s.a + ((rnd() & 1u) ? rnd() % len : rnd() % (len < 64 ? len : 64));
                if (kind < 3) d[at] = (uint8_t)rnd();
                else if (kind < 6) d[at] ^= (uint8_t)(1u << (rnd() % 8u));
                else if (kind == 6) { // the stream cut short: the chunk keeps its place, its length shrinks
                    const size_t cut = s.b - at;
                    if (cut >= len) continue;
                    const uint32_t nl = (uint32_t)(len - cut);
                    d[s.a - 8] = (uint8_t)(nl >> 24); d[s.a - 7] = (uint8_t)(nl >> 16); d[s.a - 6] = (uint8_t)(nl >> 8); d[s.a - 5] = (uint8_t)nl;
                    d.erase(d.begin() + (long)at, d.begin() + (long)s.b);
                    break;
                } else d[at] = (uint8_t)(rnd() & 1u ? 0xffu : 0u);
            }
            repair_crcs(d);
            const int r = run(d);
            if (r == 2) { printf("file %s mutant %d: the twin accepted what the host inflate refuses (or other bytes)\n", argv[a], m); return 1; }
            if (r == 1) ++refused; else ++accepted;
        }
        printf("file %s intact=%s mutants=%d refused=%d accepted=%d\n", argv[a], intact ? "ok" : "FAILED", n, refused, accepted);
        if (!intact) return 1;
    }
    return 0;
}
