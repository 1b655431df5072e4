// A GIF file through the C++ mirror (include/fanlin_gpu.hpp).
//   gif_src_host <file.gif>            prints what handler::State::gif_info says about the file (no device needed)
//   gif_src_host <file.gif> <query>    additionally runs State::process_gif and prints kind, frames and size
#include <cstdio>
#include <cstring>

#include "fanlin_gpu.hpp"

using namespace fanlin;

#define EXPECT(...) do { if (!(__VA_ARGS__)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: gif_src_host <file.gif> [query]\n"); return 2; }
    static_assert(sizeof(flgpu_gif_info) == 48, "flgpu_gif_info: eight u32, one u64, two u32");
    std::vector<uint8_t> file;
    FILE *f = std::fopen(argv[1], "rb");
    EXPECT(f != nullptr);
    uint8_t buf[4096];
    for (size_t k; (k = std::fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + k);
    std::fclose(f);
    flgpu_gif_info info;
    EXPECT(handler::State::gif_info(file, info));
    std::printf("width=%u height=%u frames=%u has_global_table=%u interlaced_frames=%u transparent_frames=%u disposal_mask=%u max_code_size=%u decoded_bytes=%llu supported=%u\n",
                info.width, info.height, info.frames, info.has_global_table, info.interlaced_frames, info.transparent_frames, info.disposal_mask,
                info.max_code_size, (unsigned long long)info.decoded_bytes, info.supported);
    if (argc < 3) return 0;
    handler::State state;
    uint32_t frames = 0;
    auto r = state.process_gif(file, query::Query::parse(argv[2]), frames);
    std::printf("kind=%d frames=%u bytes=%zu\n", (int)r.kind, frames, r.data.size());
    return 0;
}
