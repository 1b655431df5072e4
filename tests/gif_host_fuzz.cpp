// gif_host_fuzz.cpp -- the host half of the GIF decode front end (csrc/fl_gifsrc.cpp) under seeded mutations.
// A stand-alone program: tests/test_gif_source_host.py compiles it together with fl_gifsrc.cpp with
// -fsanitize=address,undefined and runs it on the CPU.  usage: gif_host_fuzz <mutations per file> <file>...
// For every file: the intact file must decode; then N mutants (byte overwrites, bit flips, truncations with the trailer put
// back, edits of the size fields of the logical screen and of the first image descriptor) go through gif_parse_info and
// gif_decode_blob, whose buffer has exactly the capacity gif_blob_capacity asks for (a write past it is a heap overflow the
// sanitizer reports) and is pre-filled: a byte changed beyond the blob's total_bytes is a wrong result, and so is a record that
// would let the device read outside the blob or write outside the canvas.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fl_gifsrc.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

// 0 = decoded into a sound blob, 1 = refused with a clean error code, 2 = a wrong result
static int run(const std::vector<uint8_t> &d)
{
    std::vector<uint8_t> file(d); // an exact-size copy: a read past the file's end is a heap overflow too
    fl::GifInfo info;
    if (fl::gif_parse_info(file.data(), file.size(), info) != 0) return 1;
    if (!info.supported) return fl::gif_decode_blob(file.data(), file.size(), nullptr, 0, nullptr) == fl::kGifUnsupported ? 1 : 2;
    if (info.decoded_bytes > fl::kGifMaxDecoded || info.frames > fl::kGifMaxFrames) return 2;
    const size_t cap = fl::gif_blob_capacity(info);
    if (cap > ((size_t)64 << 20)) return 1; // (the fuzzer keeps its heap small)
    uint8_t *blob = static_cast<uint8_t *>(aligned_alloc(16, (cap + 15u) & ~(size_t)15u));
    memset(blob, 0xa5, cap);
    fl::GifBlobHeader H;
    const int rc = fl::gif_decode_blob(file.data(), file.size(), blob, cap, &H);
    int result = 1;
    if (rc == 0) {
        result = 0;
        if (H.magic != fl::kGifMagic || H.width != info.width || H.height != info.height || H.frames != info.frames || H.total_bytes > cap ||
            H.pal_off + 1024ull * H.palettes != H.total_bytes || H.idx_off != sizeof(H) + sizeof(fl::GifFrameRec) * (size_t)H.frames || (H.pal_off & 15u)) result = 2;
        for (size_t i = H.total_bytes; i < cap && result == 0; ++i) if (blob[i] != 0xa5) result = 2;
        for (uint32_t f = 0; f < H.frames && result == 0; ++f) {
            fl::GifFrameRec r;
            memcpy(&r, blob + sizeof(H) + sizeof(r) * (size_t)f, sizeof(r));
            if (!r.w || !r.h || (uint64_t)r.x + r.w > H.width || (uint64_t)r.y + r.h > H.height || r.disposal > 7u || r.interlaced > 1u ||
                r.idx_off < H.idx_off || (uint64_t)r.idx_off + (uint64_t)r.w * r.h > H.pal_off || r.pal_off < H.pal_off || (r.pal_off & 15u) ||
                (uint64_t)r.pal_off + 1024u > H.total_bytes) result = 2;
        }
    } else if (rc != fl::kGifParse && rc != fl::kGifUnsupported) result = 2; // (kGifSmall cannot be: the capacity is the one asked for)
    free(blob);
    return result;
}

static void put16(std::vector<uint8_t> &d, size_t at, uint32_t v)
{
    if (at + 2 <= d.size()) { d[at] = (uint8_t)v; d[at + 1] = (uint8_t)(v >> 8); }
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
        // the first image descriptor, for the edits of its fields
        size_t desc = 0;
        for (size_t i = 13; i + 10 < orig.size() && !desc; ++i) if (orig[i] == 0x2c) desc = i;
        int refused = 0, wrong = 0;
        rng_state = 0x9e3779b97f4a7c15ull + (uint64_t)a;
        for (int m = 0; m < n; ++m) {
            std::vector<uint8_t> d(orig);
            const uint32_t kind = rnd() % 10u, edits = 1u + rnd() % 3u;
            for (uint32_t e = 0; e < edits; ++e) {
                const size_t at = rnd() % d.size();
                if (kind < 3) d[at] = (uint8_t)rnd();
                else if (kind < 6) d[at] ^= (uint8_t)(1u << (rnd() % 8u));
                else if (kind == 6) { d.resize(at ? at : 1); if (rnd() & 1u) { d.push_back(0); d.push_back(0x3b); } break; }
                else if (kind == 7) put16(d, 6 + 2 * (rnd() & 1u), (rnd() & 3u) ? 1u + rnd() % 64u : rnd());             // the canvas
                else if (kind == 8) put16(d, desc + 1 + 2 * (rnd() & 3u), (rnd() & 3u) ? rnd() % 24u : rnd());             // the first frame's rectangle
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
