// fl_gifdec.h -- device half of the GIF decode front end (fl_gifdec.hip): palette lookup, de-interlacing and the
// disposal / compositing chain over the blob the host half (fl_gifsrc.h) leaves, down to one composited Rgba8 canvas per frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_gifsrc.h"

namespace fl {

// Shape of gif_compose_kernel: a thread owns kGcPixels consecutive canvas pixels of one row and walks the frames.
constexpr uint32_t kGcPixels = 4, kGcThreads = 256;

// blob: the DEVICE copy of what gif_decode_blob left (16-byte aligned); out: frames x height x width Rgba8 pixels, frame after
// frame (16-byte aligned).  width, height and frames are the blob header's.
hipError_t launch_gif_compose(const uint8_t *blob, uint32_t width, uint32_t height, uint32_t frames, uint8_t *out, hipStream_t st);

} // namespace fl
