// fl_pngdec.hip -- device half of the PNG decode front end: the row filters undone, palette / sub-byte / tRNS pictures expanded.
//
// Reconstruction is Recon(x) = Filt(x) + pred(Recon(x - bpp), Up(x), Up(x - bpp)) mod 256 per byte: Sub, Average and Paeth are
// serial along a row, Up, Average and Paeth down the picture.  What is parallel is the anti-diagonal: pixel x of row y needs
// pixel x - 1 of its own row and pixels x - 1, x of the row above, so row y may run one pixel behind row y - 1.
//
// png_unfilter_kernel: one workgroup per picture, kPdWaves waves.  A wave owns a band of 64 rows: lane r reconstructs pixel
// t - r of row r at step t, keeps its own previous pixel in registers and takes the pixel above from lane r - 1 (__shfl_up;
// above-left is what it took one step earlier).  All five predictors are computed and one selected by the row's filter byte:
// no divergent branch in the step.  A band is walked in chunks of kPdChunk steps: the wave stages its slice of the chunk --
// for row r the bytes of pixels [64 j - r, 64 j - r + 64) -- into LDS with coalesced dword loads, one row per lane, reconstructs
// in place, and writes the slice back with coalesced dword stores.  The last row of a band is the "row above" of the next band's lane 0: that wave
// reads it back from the output, 64 pixels per chunk, kPdLag = 2 chunk steps behind (lane 63 finishes pixel 64 j + 64 in
// chunk j + 1).  Band b runs on wave b % 8; with more than 8 bands wave 0 continues with band 8 once it is free and band 7 is
// two chunks ahead, and so on.  Every wave runs the same number of chunk steps with one __syncthreads() each (idle steps
// included): no spin waits, no flags, nothing between workgroups.
#include "fl_pngdec.h"

#include <algorithm>
#include <atomic>

#include "fl_types.h"

namespace fl {

namespace {

typedef uint32_t __attribute__((aligned(1))) u32_unaligned; // (gfx950 loads and stores a dword at any byte address)

// stores of another wave of this workgroup, made visible by __threadfence() + __syncthreads(): read past the vector L1
__device__ __forceinline__ uint32_t load_coherent(const uint8_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LDS traffic inside one wave (staging by all lanes, then each lane on its own row): instructions of a wave execute in
// order, the compiler must keep them so
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <uint32_t BPP> __device__ __forceinline__ uint32_t lds_load_pixel(const uint8_t *p)
{
    if constexpr (BPP == 4) return *reinterpret_cast<const uint32_t *>(p);
    else if constexpr (BPP == 2) return *reinterpret_cast<const uint16_t *>(p);
    else if constexpr (BPP == 3) return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    else return p[0];
}
template <uint32_t BPP> __device__ __forceinline__ void lds_store_pixel(uint8_t *p, uint32_t v)
{
    if constexpr (BPP == 4) *reinterpret_cast<uint32_t *>(p) = v;
    else if constexpr (BPP == 2) *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    else if constexpr (BPP == 3) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); }
    else p[0] = (uint8_t)v;
}

// one pixel: f = filtered bytes, a = left, b = above, c = above-left (BPP bytes each, packed)
template <uint32_t BPP> __device__ __forceinline__ uint32_t recon_pixel(uint32_t ftype, uint32_t f, uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t out = 0;
#pragma unroll
    for (uint32_t k = 0; k < BPP; ++k) {
        const int32_t fa = (int32_t)((a >> (8u * k)) & 255u), fb = (int32_t)((b >> (8u * k)) & 255u), fc = (int32_t)((c >> (8u * k)) & 255u);
        const int32_t pa = abs(fb - fc), pb = abs(fa - fc), pc = abs(fa + fb - 2 * fc);
        const int32_t paeth = (pa <= pb && pa <= pc) ? fa : (pb <= pc ? fb : fc);
        const int32_t avg = (fa + fb) >> 1;
        int32_t pred = 0;
        pred = ftype == 1u ? fa : pred;
        pred = ftype == 2u ? fb : pred;
        pred = ftype == 3u ? avg : pred;
        pred = ftype == 4u ? paeth : pred;
        out |= (((f >> (8u * k)) + (uint32_t)pred) & 255u) << (8u * k);
    }
    return out;
}

template <uint32_t BPP> __global__ __launch_bounds__(kPdThreads) void png_unfilter_kernel(const PngDecJob *__restrict__ jobs)
{
    extern __shared__ __align__(16) uint8_t s_png[];
    constexpr uint32_t PITCH = png_lds_pitch(BPP);
    const PngDecJob &J = jobs[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t h = J.height, rb = J.row_bytes;
    const size_t stride = (size_t)rb + 1u;
    const uint8_t *__restrict__ scan = J.blob + sizeof(PngBlobHeader) + J.scan_off; // (a pass of an Adam7 picture: a picture of its own, no row above its first)
    uint8_t *out = J.rows;
    const uint32_t ns = rb / BPP;                                      // steps (pixels) per row: row_bytes is a multiple of BPP
    const uint32_t nc = (ns + 2u * kPdChunk - 2u) / kPdChunk;        // chunk steps per band: lane 63 reaches pixel ns - 1 at step ns + 62
    const uint32_t round = max(nc, kPdLag * kPdWaves);               // chunk steps between a wave's consecutive bands
    const uint32_t nbands = (h + kPdBandRows - 1u) / kPdBandRows;
    const uint32_t last = nbands - 1u;
    const uint32_t trips = (last / kPdWaves) * round + kPdLag * (last % kPdWaves) + nc; // the last band's last chunk step: the same count for every wave
    uint8_t *wbase = s_png + (size_t)wave * kPdBandRows * PITCH;
    uint8_t *mine = wbase + (size_t)lane * PITCH;
    uint32_t left = 0, corner = 0, cur = 0, ftype = 0;
    constexpr uint32_t ND = kPdChunk * BPP / 4u, RP = 64u / ND, UN = 8u; // dwords of a row's slice, rows per pass, passes whose loads are in flight together
    const uint32_t sub = lane / ND, dw = lane % ND;
    const bool lane_on = sub < RP;                                        // (bpp 3: 48 of the 64 lanes move a dword)

    for (uint32_t s = 0; s < trips; ++s) {
        // which band and chunk this wave is at (wave-uniform)
        const bool started = s >= kPdLag * wave;
        const uint32_t local = started ? s - kPdLag * wave : 0u;
        const uint32_t j = local % round, band = (local / round) * kPdWaves + wave;
        if (started && j < nc && band < nbands) {
            const uint32_t row0 = band * kPdBandRows, row = row0 + lane;
            const uint32_t nrows = min(kPdBandRows, h - row0);
            if (j == 0u) {
                left = corner = cur = 0u;
                ftype = row < h ? (uint32_t)scan[(size_t)row * stride] : 0u;
            }
            // ---- stage this chunk's slice of every row: row r holds the bytes of pixels [64 j - r, 64 j - r + 64), 16 BPP dwords.
            // A lane moves one dword (gfx950 loads and stores a dword at any byte address); 64 / ND rows go in one pass, eight passes'
            // loads are issued before the first LDS store, so their latencies overlap.  Dwords that straddle a row's end go bytewise.
            for (uint32_t r0 = 0; r0 < nrows; r0 += UN * RP) {
                uint32_t v[UN];
#pragma unroll
                for (uint32_t k = 0; k < UN; ++k) {
                    const uint32_t r = r0 + k * RP + sub;
                    const int64_t g = ((int64_t)kPdChunk * j - r) * (int64_t)BPP + 4u * dw;
                    const bool full = lane_on && r < nrows && g >= 0 && g + 4 <= (int64_t)rb;
                    v[k] = full ? *reinterpret_cast<const u32_unaligned *>(scan + (size_t)(row0 + r) * stride + 1u + g) : 0u;
                }
#pragma unroll
                for (uint32_t k = 0; k < UN; ++k) {
                    const uint32_t r = r0 + k * RP + sub;
                    const int64_t g = ((int64_t)kPdChunk * j - r) * (int64_t)BPP + 4u * dw;
                    if (!lane_on || r >= nrows) continue;
                    uint8_t *to = wbase + r * PITCH + 4u * dw;
                    if (g >= 0 && g + 4 <= (int64_t)rb) *reinterpret_cast<uint32_t *>(to) = v[k];
                    else if (g + 4 > 0 && g < (int64_t)rb) {
                        const uint8_t *src = scan + (size_t)(row0 + r) * stride + 1u;
                        for (int64_t b = 0; b < 4; ++b) if (g + b >= 0 && g + b < (int64_t)rb) to[b] = src[g + b];
                    }
                }
            }
            // ---- the row above lane 0: pixels [64 j, 64 j + 64) of the previous band's last row, one per lane
            uint32_t above = 0;
            if (row0 > 0u) {
                const uint32_t x = kPdChunk * j + lane;
                if (x < ns) {
                    const uint8_t *p = out + (size_t)(row0 - 1u) * rb + (size_t)x * BPP;
#pragma unroll
                    for (uint32_t k = 0; k < BPP; ++k) above |= load_coherent(p + k) << (8u * k);
                }
            }
            wave_lds_sync();
            // ---- kPdChunk steps of the anti-diagonal
            const bool row_ok = row < h;
#pragma unroll 4
            for (uint32_t i = 0; i < kPdChunk; ++i) {
                const uint32_t from_above = __shfl_up(cur, 1, 64), top = __shfl(above, (int)i, 64);
                const uint32_t up = lane == 0u ? top : from_above;
                const int64_t x = (int64_t)kPdChunk * j + i - lane;
                if (row_ok && x >= 0 && x < (int64_t)ns) {
                    const uint32_t f = lds_load_pixel<BPP>(mine + i * BPP);
                    cur = recon_pixel<BPP>(ftype, f, left, up, corner);
                    lds_store_pixel<BPP>(mine + i * BPP, cur);
                }
                left = cur;
                corner = up;
            }
            wave_lds_sync();
            // ---- write the slices back, a dword per lane
            for (uint32_t r0 = 0; r0 < nrows; r0 += RP) {
                const uint32_t r = r0 + sub;
                const int64_t g = ((int64_t)kPdChunk * j - r) * (int64_t)BPP + 4u * dw;
                if (!lane_on || r >= nrows) continue;
                const uint8_t *from = wbase + r * PITCH + 4u * dw;
                uint8_t *dst = out + (size_t)(row0 + r) * rb;
                if (g >= 0 && g + 4 <= (int64_t)rb) *reinterpret_cast<u32_unaligned *>(dst + g) = *reinterpret_cast<const uint32_t *>(from);
                else if (g + 4 > 0 && g < (int64_t)rb)
                    for (int64_t b = 0; b < 4; ++b) if (g + b >= 0 && g + b < (int64_t)rb) dst[g + b] = from[b];
            }
        }
        __threadfence();   // the band's last row is read by another wave, from memory
        __syncthreads();
    }
}

// What a picture's header says about its samples: the same for every pixel of a job.
struct PngSampleKind {
    uint32_t ct, d, ch, trns;
    uint32_t per, mask, scale; // samples per byte, the sample's bits, 255 / 85 / 17 / 1
};
__device__ __forceinline__ PngSampleKind png_sample_kind(const PngBlobHeader *__restrict__ H)
{
    PngSampleKind K;
    K.ct = H->color_type; K.d = H->bit_depth; K.ch = H->channels; K.trns = H->has_trns;
    K.per = 8u / K.d; K.mask = (1u << K.d) - 1u; K.scale = 255u / K.mask;
    return K;
}

// One pixel, for png_expand_kernel and png_adam7_kernel alike: sample x of an unfiltered row -> Luma8 / LumaA8 / Rgb8 / Rgba8 at o.
// Grey samples are scaled x255 / x85 / x17, the tRNS key is compared on the raw sample, the palette (256 entries, tRNS
// folded in, entries beyond PLTE opaque black) is read from the header; 8-bit colour types are copied (png_expand_kernel meets
// those only with a key; png_adam7_kernel without one too, and grey + alpha and RGBA).
__device__ __forceinline__ void png_expand_sample(const PngBlobHeader *__restrict__ H, const PngSampleKind &K, const uint8_t *__restrict__ row, uint32_t x, uint8_t *__restrict__ o)
{
    if (K.ct == 2u) { // Rgb8 (+ key)
        const uint32_t r = row[3u * x], g = row[3u * x + 1u], b = row[3u * x + 2u];
        o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
        if (K.ch == 4u) o[3] = (r == H->key[0] && g == H->key[1] && b == H->key[2]) ? 0u : 255u;
        return;
    }
    if (K.ct == 6u) { o[0] = row[4u * x]; o[1] = row[4u * x + 1u]; o[2] = row[4u * x + 2u]; o[3] = row[4u * x + 3u]; return; }
    if (K.ct == 4u) { o[0] = row[2u * x]; o[1] = row[2u * x + 1u]; return; }
    const uint32_t byte = row[x / K.per];
    const uint32_t v = (byte >> (8u - K.d * (x % K.per + 1u))) & K.mask;
    if (K.ct == 3u) {
        const uint32_t e = H->palette[v];
        o[0] = (uint8_t)e; o[1] = (uint8_t)(e >> 8); o[2] = (uint8_t)(e >> 16);
        if (K.ch == 4u) o[3] = (uint8_t)(e >> 24);
    } else {
        o[0] = (uint8_t)(v * K.scale);
        if (K.trns) o[1] = v == H->key[0] ? 0u : 255u;
    }
}

// One thread per output pixel: the unfiltered rows of a palette, sub-byte or tRNS picture -> pixels.
__global__ __launch_bounds__(256) void png_expand_kernel(const PngDecJob *__restrict__ jobs)
{
    const PngDecJob &J = jobs[blockIdx.y];
    const PngBlobHeader *__restrict__ H = reinterpret_cast<const PngBlobHeader *>(J.blob);
    const uint32_t w = J.width, rb = J.row_bytes;
    const uint32_t npx = w * J.height; // below 2^31 (png_parse_info)
    const PngSampleKind K = png_sample_kind(H);
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < npx; p += gridDim.x * 256u) {
        const uint32_t y = p / w, x = p - y * w;
        png_expand_sample(H, K, J.rows + (size_t)y * rb, x, J.pixels + (size_t)p * K.ch);
    }
}

// The pass of pixel (x & 7, y & 7) (fl_png_adam7.h)
__constant__ Adam7Map c_adam7_map = adam7_map();

// An Adam7 picture put together: one thread per output pixel, as above, but the sample comes from the unfiltered rows of the pass
// the pixel belongs to -- pass (x & 7, y & 7) of the table, there sample ((x - x0) / dx, (y - y0) / dy).  The seven passes' sizes
// and offsets are worked out once per workgroup (adam7_pass, the function the host cut the unfilter jobs with) and kept in LDS.
// Stores are coalesced as png_expand_kernel's are; loads are a strided gather inside the pass rows (an odd picture row reads one
// row of pass 7, an even one rows of up to four passes).  This kernel runs for every Adam7 picture, 8-bit ones without a key
// included: their unfiltered rows are not yet the picture.
__global__ __launch_bounds__(256) void png_adam7_kernel(const PngDecJob *__restrict__ jobs)
{
    __shared__ Adam7Pass s_pass[kAdam7Passes];
    const PngDecJob &J = jobs[blockIdx.y];
    const PngBlobHeader *__restrict__ H = reinterpret_cast<const PngBlobHeader *>(J.blob);
    const uint32_t w = J.width;
    const uint32_t npx = w * J.height; // below 2^31 (png_parse_info)
    const PngSampleKind K = png_sample_kind(H);
    if (threadIdx.x < kAdam7Passes) s_pass[threadIdx.x] = adam7_pass(w, J.height, png_pixel_bits(*H), threadIdx.x);
    __syncthreads();
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < npx; p += gridDim.x * 256u) {
        const uint32_t y = p / w, x = p - y * w;
        const uint32_t pass = c_adam7_map.pass[8u * (y & 7u) + (x & 7u)];
        const Adam7Geom G = adam7_geom(pass);
        const uint32_t px = (x - G.x0) >> G.sx, py = (y - G.y0) >> G.sy;
        const Adam7Pass &P = s_pass[pass];
        png_expand_sample(H, K, J.rows + P.rows_off + (size_t)py * P.row_bytes, px, J.pixels + (size_t)p * K.ch);
    }
}

template <uint32_t BPP> hipError_t launch_unfilter_bpp(const PngDecJob *jobs, uint32_t n, hipStream_t st)
{
    static std::atomic<uint64_t> lds_set{0};
    if (!n) return hipSuccess;
    const hipError_t e = set_max_lds_once(lds_set, (int)png_lds_bytes(BPP), {(const void *)png_unfilter_kernel<BPP>});
    if (e != hipSuccess) return e;
    png_unfilter_kernel<BPP><<<dim3(n), dim3(kPdThreads), png_lds_bytes(BPP), st>>>(jobs);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace

hipError_t launch_png_unfilter(const PngDecJob *jobs, const uint32_t njobs_bpp[4], hipStream_t st)
{
    hipError_t e;
    if ((e = launch_unfilter_bpp<1>(jobs, njobs_bpp[0], st)) != hipSuccess) return e;
    jobs += njobs_bpp[0];
    if ((e = launch_unfilter_bpp<2>(jobs, njobs_bpp[1], st)) != hipSuccess) return e;
    jobs += njobs_bpp[1];
    if ((e = launch_unfilter_bpp<3>(jobs, njobs_bpp[2], st)) != hipSuccess) return e;
    jobs += njobs_bpp[2];
    return launch_unfilter_bpp<4>(jobs, njobs_bpp[3], st);
}

hipError_t launch_png_expand(const PngDecJob *jobs, uint32_t njobs, uint32_t max_pixels, hipStream_t st)
{
    const uint32_t gx = std::min<uint32_t>(std::max<uint32_t>((max_pixels + 255u) / 256u, 1u), 4096u);
    for (uint32_t base = 0; base < njobs; base += 32768u) { // grid.y limit
        const uint32_t cnt = std::min<uint32_t>(32768u, njobs - base);
        png_expand_kernel<<<dim3(gx, cnt), dim3(256), 0, st>>>(jobs + base);
        FL_LAUNCH_CHECK();
    }
    return hipSuccess;
}

hipError_t launch_png_adam7(const PngDecJob *jobs, uint32_t njobs, uint32_t max_pixels, hipStream_t st)
{
    const uint32_t gx = std::min<uint32_t>(std::max<uint32_t>((max_pixels + 255u) / 256u, 1u), 4096u);
    for (uint32_t base = 0; base < njobs; base += 32768u) { // grid.y limit
        const uint32_t cnt = std::min<uint32_t>(32768u, njobs - base);
        png_adam7_kernel<<<dim3(gx, cnt), dim3(256), 0, st>>>(jobs + base);
        FL_LAUNCH_CHECK();
    }
    return hipSuccess;
}

} // namespace fl
