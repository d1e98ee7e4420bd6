// JPEG reconstruction on the device (akz_jpeg.hip) and the coefficient stage of the host decoder (akz_image.cpp) that feeds it.
// The host keeps marker parsing and Huffman decoding; dequantisation, IDCT, chroma upsampling, YCbCr->RGB and to_luma run
// as k_jpeg_idct + k_jpeg_luma and give the bytes of akz_image_load_luma (akz_jpeg_api.cpp: the C ABI around them).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace akz {
namespace img {
namespace jpg {

// One component of a decoded frame as the reconstruction needs it.  Its coefficients are bw * bh blocks of 64 int16 in
// natural order (row-major block grid), starting at block `blk0` of the frame's coefficient storage; its plane is
// (bw * 8) x (bh * 8) u8 samples, row stride pw = bw * 8, at byte `plane_off` of the frame's plane storage, `plane_len`
// = pw * bh * 8 bytes long, all of them written by the IDCT.  The upsampler reads no sample beyond column cwpx - 1 or row
// chpx - 1 of a subsampled component, and none beyond the frame's width and height of one at the frame's own factors.
struct FrameComp {
    uint32_t h, v, bw, bh, pw, cwpx, chpx, blk0;
    uint64_t plane_off, plane_len;
    uint16_t q[64];  // dequantisation table, natural order
};
struct Frame {
    uint32_t width, height, hmax, vmax, nc, nblocks;
    FrameComp c[3];
    uint64_t plane_bytes;  // sum of plane_len (each a multiple of 64)
};

// Storage for the coefficients: called once per stream, after the frame header, with the frame's layout (coefficient count
// = frame.nblocks * 64); returns zeroed-or-not memory for them (the decoder zeroes it), or nullptr with the status in *st
// (an error message already set) to stop the decode.
using CoefAlloc = std::function<int16_t*(const Frame& f, int* st)>;

// Part one: markers and entropy decoding of a JPEG stream into the caller's coefficient storage.  Every error the host
// decoder reports is reported here, with the same status and message, before any reconstruction.
int decode_coefs(const uint8_t* d, size_t n, const CoefAlloc& alloc, Frame& f);
// Part two on the host: what akz_image_load decodes (ch = 1: luma, 3: RGB), from the coefficients of part one.
void reconstruct_host(const Frame& f, const int16_t* coef, uint32_t* ch, std::vector<uint8_t>& px);

}  // namespace jpg

// read a whole file (false: cannot be opened / read)
bool read_file(const char* path, std::vector<uint8_t>& out);
// akz_image_load_luma on bytes already read (any supported format); path: for messages
int load_luma_bytes(const char* path, const std::vector<uint8_t>& d, uint32_t* w, uint32_t* h, std::vector<uint8_t>& luma);
inline bool is_jpeg(const std::vector<uint8_t>& d) { return d.size() >= 3 && d[0] == 0xff && d[1] == 0xd8; }
}  // namespace img

namespace launch {
// k_jpeg_idct: dequantise + IDCT every block of the frame (coefficients at d_coef) into the component planes at d_plane
void jpeg_idct(hipStream_t s, const img::jpg::Frame& f, const int16_t* d_coef, uint8_t* d_plane);
// k_jpeg_luma: upsampling, YCbCr->RGB and to_luma (or the cropped Y plane) into d_luma, width x height row-major
void jpeg_luma(hipStream_t s, const img::jpg::Frame& f, const uint8_t* d_plane, uint8_t* d_luma);
}  // namespace launch
}  // namespace akz
