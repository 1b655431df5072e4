// jpeg_opt_host.cpp -- the table rule of FLGPU_FEO_JPEG_OPTIMIZE (csrc/fl_jpeg_opt_core.h) as a program of its own, so that it can run
// under ASan + UBSan: tests/test_jpeg_optimize_host.py builds it plain and sanitised and compares what it writes with the model.
//   jpeg_opt_host IN OUT [--fallback]
// IN: K records of uint32 counts[4][256].  OUT, per record: uint32 luts[4][256], uint32 dht_bytes, uint32 optimized, uint8 dht[1108].
// Every record's invariants are checked here too: a used symbol has a length of 1..16, an unused one none; no code is all ones; the
// Kraft sum is at most 2^16 - 1 in units of 2^-16; codes of one table are distinct prefixes of nothing else (canonical order).
#include <cstdio>
#include <cstring>
#include <vector>

#include "fl_jpeg_opt_core.h"

static int check(const uint32_t *counts, const uint32_t *luts)
{
    for (int t = 0; t < 4; ++t) {
        uint64_t kraft = 0;
        for (int s = 0; s < 256; ++s) {
            const uint32_t e = luts[256 * t + s], len = e >> 16, code = e & 0xffffu;
            if ((counts[256 * t + s] != 0) != (len != 0)) return 1;
            if (!len) continue;
            if (len > 16 || code >= (1u << len) || code == (1u << len) - 1u) return 2;
            kraft += 1ull << (16 - len);
            for (int r = 0; r < s; ++r) {                       // prefix-free
                const uint32_t f = luts[256 * t + r], fl = f >> 16, fc = f & 0xffffu;
                if (!fl) continue;
                const uint32_t m = fl < len ? fl : len;
                if ((code >> (len - m)) == (fc >> (fl - m))) return 3;
            }
        }
        if (kraft > 65535u) return 4;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const bool fallback = argc > 3 && !strcmp(argv[3], "--fallback");
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<uint32_t> counts(1024), luts(1024);
    std::vector<uint8_t> dht(1108);
    int records = 0;
    while (fread(counts.data(), 4, 1024, in) == 1024) {
        uint32_t n = 0;
        memset(dht.data(), 0, dht.size());
        const int on = fl::jpeg_opt_tables_serial(counts.data(), fallback, luts.data(), dht.data(), &n);
        if (on < 0) { fprintf(stderr, "record %d: counts out of range\n", records); return 1; }
        if (const int bad = check(counts.data(), luts.data())) { fprintf(stderr, "record %d: invariant %d broken\n", records, bad); return 1; }
        const uint32_t tail[2] = {n, (uint32_t)on};
        fwrite(luts.data(), 4, 1024, out);
        fwrite(tail, 4, 2, out);
        fwrite(dht.data(), 1, dht.size(), out);
        ++records;
    }
    fclose(in);
    fclose(out);
    printf("jpeg_opt ok %d records\n", records);
    return 0;
}
