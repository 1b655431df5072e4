// fl_gifdec.hip -- device half of the GIF decode front end: every composited frame of an animation from the blob of records,
// palettes and index bytes the host half leaves (fl_gifsrc.h).
//
// The compositing rule is image 0.25.6's GifFrameIterator::next / blend_and_dispose_pixel, restated from memory (DESIGN.md
// section 4): a frame's pixel replaces the canvas pixel unless its alpha is 0, the composited canvas is the frame handed out,
// and the frame's disposal method says what the NEXT frame is drawn over -- the composited canvas (0, 1 and 4..7), the canvas
// with the frame's rectangle cleared to 0, 0, 0, 0 (2), or the canvas as it was before the frame (3).
//
// gif_compose_kernel: the chain is sequential over frames and independent per canvas pixel, so one thread owns kGcPixels
// consecutive pixels of one canvas row and walks frames 0 .. F - 1 with two dwords of state per pixel: `prev`, what the next
// frame is drawn over, and `cur`, the frame handed out.  A frame's record is the same for every lane (scalar loads through a
// const pointer); inside its rectangle a lane reads one index byte per pixel -- the stored row from the four-pass interlace
// map where the frame is interlaced -- and looks it up in the frame's palette, 1 KB that stays in the vector L1.  Every frame's
// pixels leave in one 16-byte store where the canvas width is a multiple of four.  No LDS, no barrier, no waiting between
// waves or workgroups: the kernel is bound by its F x W x H x 4 bytes of stores, the indices are read once.
#include "fl_gifdec.h"

#include "fl_types.h"

namespace fl {

namespace {

// The stored row (position in the file's row order) of row r of an interlaced frame of h rows: rows 0, 8, .. first, then
// 4, 12, .., then 2, 6, .., then 1, 3, ..
__device__ __forceinline__ uint32_t gif_stored_row(uint32_t r, uint32_t h)
{
    const uint32_t n1 = (h + 7u) >> 3, n2 = (h + 3u) >> 3, n3 = (h + 1u) >> 2;
    if ((r & 7u) == 0u) return r >> 3;
    if ((r & 7u) == 4u) return n1 + (r >> 3);
    if ((r & 3u) == 2u) return n1 + n2 + (r >> 2);
    return n1 + n2 + n3 + (r >> 1);
}

// kVec: width is a multiple of kGcPixels, so a thread's pixels are 16 bytes at a 16-byte boundary
template <bool kVec>
__global__ __launch_bounds__(kGcThreads) void gif_compose_kernel(const uint8_t *__restrict__ blob, uint32_t width, uint32_t height, uint32_t frames,
                                                                  uint32_t *__restrict__ out)
{
    const uint32_t qw = (width + kGcPixels - 1u) / kGcPixels;
    const uint32_t t = blockIdx.x * kGcThreads + threadIdx.x;
    if (t >= qw * height) return;
    const uint32_t y = t / qw, x0 = (t - y * qw) * kGcPixels;
    const GifFrameRec *__restrict__ recs = reinterpret_cast<const GifFrameRec *>(blob + sizeof(GifBlobHeader));
    const size_t plane = (size_t)width * height;
    uint32_t *o = out + (size_t)y * width + x0;
    uint32_t prev[kGcPixels], cur[kGcPixels];
#pragma unroll
    for (uint32_t k = 0; k < kGcPixels; ++k) prev[k] = 0u;
    for (uint32_t f = 0; f < frames; ++f, o += plane) {
        const GifFrameRec r = recs[f];
        const uint32_t ry = y - r.y; // (below the rectangle's first row this wraps to a large value)
        bool inside[kGcPixels];
#pragma unroll
        for (uint32_t k = 0; k < kGcPixels; ++k) { cur[k] = prev[k]; inside[k] = false; }
        if (ry < r.h) {
            const uint32_t srow = r.interlaced ? gif_stored_row(ry, r.h) : ry;
            const uint8_t *__restrict__ idx = blob + r.idx_off + (size_t)srow * r.w;
            const uint32_t *__restrict__ pal = reinterpret_cast<const uint32_t *>(blob + r.pal_off);
#pragma unroll
            for (uint32_t k = 0; k < kGcPixels; ++k) {
                const uint32_t dx = x0 + k - r.x;
                // the rectangle lies inside the canvas: a pixel beyond the canvas width is beyond the rectangle too
                if (dx < r.w) {
                    inside[k] = true;
                    const uint32_t colour = pal[idx[dx]];
                    if (colour >> 24) cur[k] = colour;
                }
            }
        }
        if (kVec) *reinterpret_cast<uint4 *>(o) = make_uint4(cur[0], cur[1], cur[2], cur[3]);
        else {
#pragma unroll
            for (uint32_t k = 0; k < kGcPixels; ++k)
                if (x0 + k < width) o[k] = cur[k];
        }
        // what the next frame is drawn over (outside the rectangle cur == prev)
        if (r.disposal == 2u) {
#pragma unroll
            for (uint32_t k = 0; k < kGcPixels; ++k) prev[k] = inside[k] ? 0u : prev[k];
        } else if (r.disposal != 3u) {
#pragma unroll
            for (uint32_t k = 0; k < kGcPixels; ++k) prev[k] = cur[k];
        }
    }
}

} // namespace

hipError_t launch_gif_compose(const uint8_t *blob, uint32_t width, uint32_t height, uint32_t frames, uint8_t *out, hipStream_t st)
{
    if (!frames || !width || !height) return hipSuccess;
    const uint64_t threads = (uint64_t)((width + kGcPixels - 1u) / kGcPixels) * height;
    if (threads > 0x7fffffffull) return hipErrorInvalidValue;
    const uint32_t gx = (uint32_t)((threads + kGcThreads - 1u) / kGcThreads);
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    if (width % kGcPixels == 0u) gif_compose_kernel<true><<<dim3(gx), dim3(kGcThreads), 0, st>>>(blob, width, height, frames, o);
    else gif_compose_kernel<false><<<dim3(gx), dim3(kGcThreads), 0, st>>>(blob, width, height, frames, o);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace fl
