// Frames as a caller holds them (akz_frame_layout: colour or grey, pitched, strided, cropped) -> the packed luma frames the
// extraction takes.  The ONE expression of DynamicImage::to_luma is here, as one piece of source for the host loops
// (img::to_luma in akz_image.cpp, akz_luma_from_frames_host in akz_frames_api.cpp) and for the device (k_jpeg_luma in
// akz_jpeg.hip, k_frame_luma in akz_frames.hip): three f32 products and two f32 sums in this order, never contracted
// (-ffp-contract=off on both sides), truncated to u8 -- so every path gives the same byte for the same (R, G, B).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/akaze_hip.h"

#ifndef AKZ_HD
#if defined(__HIPCC__)
#define AKZ_HD __host__ __device__ inline
#else
#define AKZ_HD inline
#endif
#endif

namespace akz {

// `image` 0.21's to_luma of one Rgb<u8> pixel (believed: f32 weights, truncating cast).  Note (v, v, v) -> v does NOT hold
// for every v (13 is the first that gives v - 1).
AKZ_HD uint8_t luma_u8(uint8_t r, uint8_t g, uint8_t b) {
    const float l = 0.2126f * (float)r + 0.7152f * (float)g + 0.0722f * (float)b;
    return (uint8_t)l;
}

// An akz_frame_layout with every 0 replaced by its tight value, checked (frames_resolve).
struct FrameSpec {
    uint32_t format = 0, w = 0, h = 0;
    uint32_t bpp = 0;  // bytes from a pixel to the next inside a row (1 for the planar format: per plane)
    uint64_t row_pitch = 0, frame_stride = 0, plane_stride = 0;
    bool packed_gray() const { return format == AKZ_FRAME_GRAY8 && row_pitch == w && frame_stride == (uint64_t)w * h; }
};
// AKZ_ERR_INVALID_ARG with the field named in akz_last_error: null src / layout, n == 0, an unknown format, a zero width or
// height, a nonzero pitch or stride below its tight value.  `who`: the entry point, for the message.
int frames_resolve(const char* who, const void* src, const akz_frame_layout* layout, uint32_t n, FrameSpec& out);

namespace launch {
// k_frame_luma<format>: d_luma[n][h][w] (packed, any alignment) = to_luma of the frames at d_src
void frame_luma(hipStream_t s, const uint8_t* d_src, const FrameSpec& fs, uint32_t n, uint8_t* d_luma);
}  // namespace launch
}  // namespace akz
