// A lossless WebP source through the C++ mirror (include/fanlin_gpu.hpp).
//   webp_src_host <file.webp>            prints what handler::State::webp_info says about the file (no device needed)
//   webp_src_host <file.webp> <query>    additionally runs State::process_webp with FLGPU_ENCODE_WEBP_LOSSLESS and prints kind and size
#include <cstdio>
#include <cstring>

#include "fanlin_gpu.hpp"

using namespace fanlin;

#define EXPECT(...) do { if (!(__VA_ARGS__)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: webp_src_host <file.webp> [query]\n"); return 2; }
    static_assert(sizeof(flgpu_webp_info) == 12 * sizeof(uint32_t), "flgpu_webp_info is twelve u32");
    static_assert(FLGPU_IMG_WEBP_SOURCE == 64u, "flag value");
    std::vector<uint8_t> file;
    FILE *f = std::fopen(argv[1], "rb");
    EXPECT(f != nullptr);
    uint8_t buf[4096];
    for (size_t k; (k = std::fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + k);
    std::fclose(f);
    flgpu_webp_info info;
    EXPECT(handler::State::webp_info(file, info));
    std::printf("width=%u height=%u channels=%u has_alpha=%u extended=%u animated=%u lossless=%u exif_orientation=%u transforms=%u color_cache_bits=%u prefix_groups=%u supported=%u\n",
                info.width, info.height, info.channels, info.has_alpha, info.extended, info.animated, info.lossless, info.exif_orientation,
                info.transforms, info.color_cache_bits, info.prefix_groups, info.supported);
    if (argc < 3) return 0;
    content::Format fmt;
    handler::State state;
    auto r = state.process_webp(file, query::Query::parse(argv[2]), fmt);
    std::printf("kind=%d bytes=%zu\n", (int)r.kind, r.data.size());
    return 0;
}
