// One PNG request through the C++ mirror (include/fanlin_gpu.hpp): a PNG input that stays PNG, with the opt-in bit, comes back
// as the finished image/png body.   png_host <out.png>  (writes the body there; the test takes it apart in Python)
#include <cstdio>
#include <cstring>

#include "fanlin_gpu.hpp"

using namespace fanlin;

#define EXPECT(...) do { if (!(__VA_ARGS__)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: png_host <out.png>\n"); return 2; }
    content::Format f;
    f.encode_png();
    EXPECT((f.flags() & FLGPU_ENCODE_PNG) != 0 && !f.webp_accepted());
    handler::State state;
    std::vector<uint8_t> px(640 * 360 * 3);
    for (uint32_t y = 0; y < 360; ++y)
        for (uint32_t x = 0; x < 640; ++x)
            for (uint32_t c = 0; c < 3; ++c) px[(y * 640 + x) * 3 + c] = (uint8_t)((x * (c + 1) + y * (3 - c)) / 3);
    handler::Decoded img{px.data(), 640, 360, 3, 1, FLGPU_IN_PNG};
    auto r = state.process_image(img, query::Query::parse("w=300&h=200"), f);
    EXPECT(r.kind == FLGPU_RESULT_PNG_STREAM && r.negotiated == FLGPU_OUT_KEEP);
    EXPECT(r.data.size() > 57 && std::memcmp(r.data.data(), "\x89PNG\r\n\x1a\n", 8) == 0);
    FILE *o = std::fopen(argv[1], "wb");
    EXPECT(o != nullptr);
    EXPECT(std::fwrite(r.data.data(), 1, r.data.size(), o) == r.data.size());
    std::fclose(o);
    content::Format plain;
    r = state.process_image(img, query::Query::parse("w=300&h=200"), plain);
    EXPECT(r.kind == FLGPU_RESULT_PIXELS && r.data.size() == 300 * 200 * 4);
    std::puts("png ok");
    return 0;
}
