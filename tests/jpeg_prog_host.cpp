// jpeg_prog_host.cpp -- the progressive coder of FLGPU_FEO_JPEG_PROGRESSIVE in plain loops (csrc/fl_jpeg_prog_core.h) as a program of its
// own, so that it can run under ASan + UBSan: tests/test_jpeg_progressive_host.py builds it plain and sanitised and compares what it
// writes with the model.
//   jpeg_prog_host IN OUT
// IN: K records of uint32 nblocks, uint8 prefix[177] (the baseline header's), 3 padding bytes, int16 coef[3 * nblocks][64].
// OUT, per record: uint32 counts[6][256], uint32 file_bytes, the file.  The destination is sized exactly: a second run into a
// destination one byte shorter must report the same length and write nothing past it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fl_jpeg_prog_core.h"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int records = 0;
    uint32_t nblocks;
    while (fread(&nblocks, 4, 1, in) == 1) {
        uint8_t prefix[180];
        if (fread(prefix, 1, 180, in) != 180) return 2;
        std::vector<int16_t> coef((size_t)nblocks * 3u * 64u);
        if (fread(coef.data(), 2, coef.size(), in) != coef.size()) return 2;
        std::vector<uint32_t> counts(fl::kJpegProgTables * 256u), again(counts.size());
        uint64_t n = 0, m = 0;
        if (fl::jpeg_prog_encode_serial(coef.data(), nblocks, prefix, counts.data(), nullptr, 0, &n)) { fprintf(stderr, "record %d: counts out of range\n", records); return 1; }
        std::vector<uint8_t> file(n), shorter(n - 1u);
        if (fl::jpeg_prog_encode_serial(coef.data(), nblocks, prefix, again.data(), file.data(), file.size(), &m) || m != n || again != counts) return 1;
        if (fl::jpeg_prog_encode_serial(coef.data(), nblocks, prefix, again.data(), shorter.data(), shorter.size(), &m) || m != n) return 1;
        if (memcmp(file.data(), shorter.data(), shorter.size())) return 1;
        const uint32_t bytes = (uint32_t)n;
        fwrite(counts.data(), 4, counts.size(), out);
        fwrite(&bytes, 4, 1, out);
        fwrite(file.data(), 1, file.size(), out);
        ++records;
    }
    fclose(in);
    fclose(out);
    printf("jpeg_prog ok %d records\n", records);
    return 0;
}
