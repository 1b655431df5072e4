// One lossless WebP request through the C++ mirror (include/fanlin_gpu.hpp): `webp=true&quality=100` from a client that accepts
// WebP, with the opt-in bit, comes back as the finished image/webp body.   webp_host <out.webp>  (writes the body there; the test
// decodes it in Python)
#include <cstdio>
#include <cstring>

#include "fanlin_gpu.hpp"

using namespace fanlin;

#define EXPECT(...) do { if (!(__VA_ARGS__)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: webp_host <out.webp>\n"); return 2; }
    content::Format f;
    f.accept_webp();
    f.encode_webp_lossless();
    EXPECT((f.flags() & FLGPU_ENCODE_WEBP_LOSSLESS) != 0 && f.webp_accepted() && (f.flags() & FLGPU_ENCODE_PNG) == 0);
    handler::State state;
    std::vector<uint8_t> px(640 * 360 * 3);
    for (uint32_t y = 0; y < 360; ++y)
        for (uint32_t x = 0; x < 640; ++x)
            for (uint32_t c = 0; c < 3; ++c) px[(y * 640 + x) * 3 + c] = (uint8_t)((x * (c + 1) + y * (3 - c)) / 3);
    handler::Decoded img{px.data(), 640, 360, 3, 1, FLGPU_IN_PNG};
    auto r = state.process_image(img, query::Query::parse("w=300&h=200&webp=true&quality=100"), f);
    EXPECT(r.kind == FLGPU_RESULT_WEBP_STREAM && r.negotiated == FLGPU_OUT_WEBP);
    EXPECT(r.data.size() > 21 && std::memcmp(r.data.data(), "RIFF", 4) == 0 && std::memcmp(r.data.data() + 8, "WEBPVP8L", 8) == 0);
    EXPECT(r.data.size() <= r.plan.max_out_bytes);
    FILE *o = std::fopen(argv[1], "wb");
    EXPECT(o != nullptr);
    EXPECT(std::fwrite(r.data.data(), 1, r.data.size(), o) == r.data.size());
    std::fclose(o);
    content::Format plain;
    plain.accept_webp();
    r = state.process_image(img, query::Query::parse("w=300&h=200&webp=true&quality=100"), plain);
    EXPECT(r.kind == FLGPU_RESULT_PIXELS && r.data.size() == 300 * 200 * 4);
    std::puts("webp ok");
    return 0;
}
