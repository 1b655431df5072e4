// fl_jpeg.hip -- the JPEG encoder's back half on gfx950: colour conversion + forward DCT + quantisation, then
// Huffman coding, byte stuffing and framing, so that what leaves the GPU is the finished JFIF stream.
//
// Replaces `JpegEncoder::new_with_quality(&mut buffer, q).encode_image(&img)` (reference src/handler.rs:274-278),
// i.e. image 0.25.6 src/codecs/jpeg/encoder.rs (encode_image, encode_rgb, BitWriter::write_block / write_bits /
// huffman_encode, build_* header helpers) and src/codecs/jpeg/transform.rs (fdct): baseline, three components,
// all sampling factors 1x1, Annex K quantisation tables scaled by quality, Annex K Huffman tables.
//
// Two kernels per batch:
//   jpeg_dct_quant_kernel   one wave per 16 consecutive blocks, in two phases.  Transform: block after block, the 64
//                           lanes are the 64 samples / coefficients.  The integer DCT of transform.rs (IJG jfdctint) is
//                           linear up to the final shift of each pass, so a lane computes ITS coefficient as an 8-term
//                           integer dot product with a constant matrix derived at compile time from the butterfly itself
//                           (int32 wrap-around arithmetic is a ring: the sums are identical bit for bit); lane k owns
//                           zig-zag coefficient k, so the quantised units land in LDS in coding order, with a ballot of
//                           their non-zero AC terms.  Coding: each lane Huffman-codes whole units on its own, walking
//                           the set bits of the unit's mask (lane 16 k + b: component k of block b).
//                           Out: one 16-byte record per unit (JpegUnit: quantised DC, AC bit count, the first 96 bits
//                           of the AC code); the rare longer code goes on in the unit's acbits slot.
//   jpeg_pack_kernel        one workgroup per picture: DC code sizes (they need the previous block) + AC sizes ->
//                           exclusive scan -> bit offset of every block; the blocks' bits are shifted into place in an
//                           LDS window of the stream (atomics), then pad_byte, 0xFF -> 0xFF00 stuffing by a second
//                           scan, header, EOI, length.  Long streams are handled window after window.  A unit costs
//                           one 16-byte load, requested a round of 512 units ahead of its use.
// HBM traffic is the pixels once (the input is the 240 KB picture the resample kernel just wrote, L2 resident) plus
// the unit records (16 bytes per unit, written and read once, consecutive within a picture); the kernels are VALU / LDS
// bound, not bandwidth bound.
// The device code itself is in fl_jpeg_dev.h, which this file shares with fl_jpeg_opt.hip (FLGPU_FEO_JPEG_OPTIMIZE: the same transform,
// coder and packer with per-picture Huffman tables); this translation unit holds the two kernels of the plain encode and nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_jpeg_dev.h"

namespace fl {

namespace {

__global__ __launch_bounds__(kJpegThreads) void jpeg_dct_quant_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                      uint32_t job_base)
{
    jpeg_code_units<false>(jobs, arena, job_base, nullptr);
}

} // namespace

hipError_t launch_jpeg_encode(const JpegJob *jobs, const uint32_t *arena, uint32_t job_base, uint32_t njobs, uint32_t max_blocks,
                              hipStream_t st)
{
    if (!njobs || !max_blocks) return hipSuccess;
    hipLaunchKernelGGL(jpeg_dct_quant_kernel, dim3((max_blocks + kBlocksPerWg - 1) / kBlocksPerWg, njobs), dim3(kJpegThreads), 0, st, jobs, arena, job_base);
    FL_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pack_kernel<false>, dim3(njobs), dim3(kPackThreads), 0, st, jobs, arena, job_base, (const uint32_t *)nullptr);
    FL_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace fl
