// JPEG reconstruction after the host's entropy decoding (akz_jpeg.hpp): k_jpeg_idct dequantises and transforms the coefficient
// blocks into padded component planes, k_jpeg_luma upsamples the chroma, converts to RGB and to luma in one pass per output
// pixel.  Both are the host decoder's arithmetic (akz_image.cpp: idct, reconstruct_host) operation for operation: the same
// 64-bit integer IDCT, the same branches of the upsampler and the same unfused f32 colour and luma expressions
// (-ffp-contract=off), so the bytes equal akz_image_load_luma's for every stream the host accepts.  The upsampler copies a
// component only at the frame's own factors (h == hmax and v == vmax), filters one at half the horizontal factor, and
// takes the nearest sample by position for every other, a factor that does not divide the maximum included.
#include <hip/hip_runtime.h>

#include "akz_frames.hpp"
#include "akz_internal.hpp"
#include "akz_jpeg.hpp"

namespace akz {
namespace {

using img::jpg::Frame;
using img::jpg::FrameComp;

constexpr int IT = 256;              // k_jpeg_idct: 8 lanes per block, 32 blocks per workgroup
constexpr int IB = IT / 8;
constexpr int LX = 256;              // k_jpeg_luma: pixels per workgroup (one row segment)

typedef int64_t I;
constexpr I f2f(double x) { return (I)(x * 4096 + 0.5); }
constexpr I c0 = f2f(0.5411961), c1 = f2f(-1.847759065), c2 = f2f(0.765366865), c3 = f2f(1.175875602), c4 = f2f(0.298631336),
            c5 = f2f(2.053119869), c6 = f2f(3.072711026), c7 = f2f(1.501321110), c8 = f2f(-0.899976223), c9 = f2f(-2.562915447),
            c10 = f2f(-1.961570560), c11 = f2f(-0.390180644);

// one 1-D pass of the stb-style IDCT (akz_image.cpp: idct's `pass`)
__device__ inline void idct_pass(I s0, I s1, I s2, I s3, I s4, I s5, I s6, I s7, I (&x)[4], I (&t)[4]) {
    I p2 = s2, p3 = s6;
    I p1 = (p2 + p3) * c0;
    I t2 = p1 + p3 * c1, t3 = p1 + p2 * c2;
    p2 = s0; p3 = s4;
    I t0 = (p2 + p3) * 4096, t1 = (p2 - p3) * 4096;
    x[0] = t0 + t3; x[3] = t0 - t3; x[1] = t1 + t2; x[2] = t1 - t2;
    t0 = s7; t1 = s5; t2 = s3; t3 = s1;
    p3 = t0 + t2;
    I p4 = t1 + t3;
    p1 = t0 + t3; p2 = t1 + t2;
    const I p5 = (p3 + p4) * c3;
    t0 = t0 * c4; t1 = t1 * c5; t2 = t2 * c6; t3 = t3 * c7;
    p1 = p5 + p1 * c8; p2 = p5 + p2 * c9; p3 = p3 * c10; p4 = p4 * c11;
    t[3] = t3 + p1 + p4; t[2] = t2 + p2 + p3; t[1] = t1 + p2 + p4; t[0] = t0 + p1 + p3;
}
__device__ inline uint32_t clamp8(I x) { return (uint32_t)(x < 0 ? 0 : (x > 255 ? 255 : x)); }

// Lane 8b + i of a workgroup: column i, then row i, of block b.  A dequantised coefficient reaches +-2^31 (int16 times a
// 16-bit table), which the 32-bit form of the transform overflows: every product and sum is 64-bit, as on the host.  The
// column results go through LDS to the lanes of the row pass (the same wave: 8 blocks per wave).
__global__ void __launch_bounds__(IT) k_jpeg_idct(Frame f, const int16_t* __restrict__ coef, uint8_t* __restrict__ plane) {
    __shared__ I s_val[IB][64];
    const uint32_t lb = threadIdx.x >> 3, i = threadIdx.x & 7;
    const uint32_t b = blockIdx.x * IB + lb;
    const bool live = b < f.nblocks;
    const int k = !live ? 0 : (f.nc > 1 && b >= f.c[1].blk0) + (f.nc > 2 && b >= f.c[2].blk0);
    const FrameComp& c = f.c[k];
    if (live) {
        const int16_t* in = coef + (size_t)b * 64;
        I dq[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) dq[r] = (I)in[i + 8 * r] * (I)c.q[i + 8 * r];
        I* v = &s_val[lb][i];
        if (!dq[1] && !dq[2] && !dq[3] && !dq[4] && !dq[5] && !dq[6] && !dq[7]) {
            const I dc = dq[0] * 4;
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r * 8] = dc;
        } else {
            I x[4], t[4];
            idct_pass(dq[0], dq[1], dq[2], dq[3], dq[4], dq[5], dq[6], dq[7], x, t);
#pragma unroll
            for (int m = 0; m < 4; ++m) x[m] += 512;
            v[0] = (x[0] + t[3]) >> 10; v[56] = (x[0] - t[3]) >> 10;
            v[8] = (x[1] + t[2]) >> 10; v[48] = (x[1] - t[2]) >> 10;
            v[16] = (x[2] + t[1]) >> 10; v[40] = (x[2] - t[1]) >> 10;
            v[24] = (x[3] + t[0]) >> 10; v[32] = (x[3] - t[0]) >> 10;
        }
    }
    __syncthreads();
    if (!live) return;
    const I* v = &s_val[lb][8 * i];
    I x[4], t[4];
    idct_pass(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], x, t);
#pragma unroll
    for (int m = 0; m < 4; ++m) x[m] += 65536 + ((I)128 << 17);
    const uint32_t o0 = clamp8((x[0] + t[3]) >> 17), o7 = clamp8((x[0] - t[3]) >> 17);
    const uint32_t o1 = clamp8((x[1] + t[2]) >> 17), o6 = clamp8((x[1] - t[2]) >> 17);
    const uint32_t o2 = clamp8((x[2] + t[1]) >> 17), o5 = clamp8((x[2] - t[1]) >> 17);
    const uint32_t o3 = clamp8((x[3] + t[0]) >> 17), o4 = clamp8((x[3] - t[0]) >> 17);
    const uint32_t kb = b - c.blk0, by = kb / c.bw, bx = kb - by * c.bw;
    // the plane starts on 8 bytes and its stride is a multiple of 8: one aligned 8-byte store per row of the block
    uint2* o = (uint2*)(plane + c.plane_off + ((size_t)by * 8 + i) * c.pw + (size_t)bx * 8);
    *o = make_uint2(o0 | o1 << 8 | o2 << 16 | o3 << 24, o4 | o5 << 8 | o6 << 16 | o7 << 24);
}

// The sample of component c that reconstruct_host puts at (x, y) of its upsampled row.
__device__ inline int upsampled(const FrameComp& c, const uint8_t* __restrict__ p, int x, int y, int width, int hmax, int vmax) {
    const int pw = (int)c.pw, sh = hmax / (int)c.h, sv = vmax / (int)c.v, cwpx = (int)c.cwpx, chpx = (int)c.chpx;
    if ((int)c.h == hmax && (int)c.v == vmax) return p[(size_t)y * pw + x];
    if (sh == 2 && (sv == 1 || sv == 2) && hmax % (int)c.h == 0 && vmax % (int)c.v == 0) {
        const int i = x >> 1;
        if (sv == 1) {  // h2v1 fancy upsampling
            const uint8_t* n = p + (size_t)y * pw;
            if (cwpx == 1) return n[0];
            if (x == 0) return n[0];
            if ((x & 1) && i == cwpx - 1) return n[cwpx - 1];
            return (x & 1) ? (3 * n[i] + n[i + 1] + 2) >> 2 : (3 * n[i] + n[i - 1] + 2) >> 2;
        }
        // h2v2: the vertical triangle first (t = 3 near + far), then the horizontal one
        const int yn = y >> 1, yf = (y & 1) ? min(yn + 1, chpx - 1) : max(yn - 1, 0);
        const uint8_t* n = p + (size_t)yn * pw;
        const uint8_t* fr = p + (size_t)yf * pw;
        if (x == 0 || x == 2 * cwpx - 1) {
            const int j = x == 0 ? 0 : cwpx - 1;
            return (3 * n[j] + fr[j] + 2) >> 2;
        }
        const int a = (x & 1) ? (x + 1) >> 1 : i;  // the centre (x odd: output 2a - 1 between a - 1 and a; even: 2a)
        const int ta = 3 * n[a] + fr[a], tb = 3 * n[a - 1] + fr[a - 1];
        return (x & 1) ? (3 * tb + ta + 8) >> 4 : (3 * ta + tb + 8) >> 4;
    }
    const int yy = min(y * (int)c.v / vmax, chpx - 1);
    return p[(size_t)yy * pw + min(x * (int)c.h / hmax, cwpx - 1)];
}
__device__ inline uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ void __launch_bounds__(LX) k_jpeg_luma(Frame f, const uint8_t* __restrict__ plane, uint8_t* __restrict__ luma) {
    const int x = (int)(blockIdx.x * LX + threadIdx.x), y = (int)blockIdx.y;
    const int width = (int)f.width;
    if (x >= width) return;
    uint8_t* o = luma + (size_t)y * width + x;
    if (f.nc == 1) {
        *o = plane[f.c[0].plane_off + (size_t)y * f.c[0].pw + x];
        return;
    }
    const int hmax = (int)f.hmax, vmax = (int)f.vmax;
    const int s0 = upsampled(f.c[0], plane + f.c[0].plane_off, x, y, width, hmax, vmax);
    const int s1 = upsampled(f.c[1], plane + f.c[1].plane_off, x, y, width, hmax, vmax);
    const int s2 = upsampled(f.c[2], plane + f.c[2].plane_off, x, y, width, hmax, vmax);
    const float Y = (float)s0, cb = (float)s1 - 128.0f, cr = (float)s2 - 128.0f;
    const float r = Y + 1.40200f * cr;
    const float g = Y - 0.34414f * cb - 0.71414f * cr;
    const float b = Y + 1.77200f * cb;
    const uint8_t R = clamp_u8((int)(r + 0.5f)), G = clamp_u8((int)(g + 0.5f)), B = clamp_u8((int)(b + 0.5f));
    *o = luma_u8(R, G, B);  // img::to_luma
}

}  // namespace

namespace launch {
void jpeg_idct(hipStream_t s, const img::jpg::Frame& f, const int16_t* d_coef, uint8_t* d_plane) {
    if (!f.nblocks) return;
    hipLaunchKernelGGL(k_jpeg_idct, dim3((f.nblocks + IB - 1) / IB), dim3(IT), 0, s, f, d_coef, d_plane);
}
void jpeg_luma(hipStream_t s, const img::jpg::Frame& f, const uint8_t* d_plane, uint8_t* d_luma) {
    if (!f.width || !f.height) return;
    hipLaunchKernelGGL(k_jpeg_luma, dim3((f.width + LX - 1) / LX, f.height), dim3(LX), 0, s, f, d_plane, d_luma);
}
}  // namespace launch
}  // namespace akz
