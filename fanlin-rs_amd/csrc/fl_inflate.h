// fl_inflate.h -- the deflate stream of a PNG source inflated on the device (fl_inflate.hip), for sources that carry
// FLGPU_IMG_PNG_INFLATE: the calling thread only walks the container and copies the IDAT payloads behind a PngBlobHeader
// (png_stage_compressed, fl_pngsrc.cpp), the compressed payload crosses PCIe, and one workgroup per picture writes the filtered
// scanlines into a scratch laid out like the blob of the host path, so the unfilter / expand / Adam7 kernels run unchanged.
// The device answers "yes, and here are the scanlines" or "no"; every "no" is run again with the host inflate, whose verdict is final.
// The strip shape is stated here (the tests read it); the data-dependent steps are in fl_inflate_core.h, shared with the host twin.
#pragma once
#include <stdint.h>

namespace fl {
// A strip of the token stream: kInfSubs subsequences of kInfSubBits bits, one per thread of the workgroup.
constexpr uint32_t kInfSubBits = 128;
constexpr uint32_t kInfSubs = 256;
} // namespace fl

#if defined(__HIPCC__) // (the rest is the launch interface; the host half and its stand-alone test programs take the constants alone)
#include <hip/hip_runtime.h>

#include "fl_inflate_core.h"
#include "fl_pngsrc.h"

namespace fl {

constexpr uint32_t kInfThreads = kInfSubs; // one thread per subsequence of a strip

// One picture of an inflate launch.
struct alignas(16) InfJob {
    const uint8_t *stage;   // device copy of what png_stage_compressed left: PngBlobHeader (magic kPngzMagic) + payload + kPngzPad zero bytes
    uint8_t *scratch;       // receives PngBlobHeader (magic kPngMagic) + the scanlines: what PngDecJob::blob points at
    uint32_t *err;          // 0 = the scanlines are whole and checked, otherwise why not (kInfErr*)
    uint32_t payload_bytes; // of the deflate stream (zlib header and check value included)
    uint32_t expected;      // bytes of the scanlines IHDR implies
};

// why the device said no (the error word; the host re-run names the defect for the caller)
enum : uint32_t {
    kInfErrZlibHeader = 1, kInfErrTruncated, kInfErrBlockType, kInfErrDynamicHeader, kInfErrStored, kInfErrCode, kInfErrTooLong,
    kInfErrDistance, kInfErrRounds, kInfErrTooShort, kInfErrAdler, kInfErrFilterByte
};

hipError_t launch_png_inflate(const InfJob *jobs, uint32_t njobs, hipStream_t st);

} // namespace fl
#endif
