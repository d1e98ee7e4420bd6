// k_frame_luma<FMT>: akz_luma_from_frames_host on the device -- n frames in one of the six akz_frame_format layouts, with a row
// pitch, a frame stride and (planar) a plane stride, to packed luma frames.  One streaming pass, 4 to 5 bytes per pixel.
//
// Access shape.  The batch's output is one flat array of n * w * h bytes at an address of any alignment.  A lane owns ONE
// NATURALLY ALIGNED 4-BYTE WORD of it -- four pixels of one row -- and a workgroup of FT lanes FT consecutive words of a row,
// counted from the aligned word that holds the row's first byte.  A word that lies wholly inside the row is written with one
// 4-byte store; the (at most three) bytes of a row in front of its first whole word and behind its last are written one by
// one, by the lane whose word they are in.  Two rows that meet inside a word each write their own bytes of it, so nothing
// but the n * w * h output bytes is ever stored.
// The 4, 12 or 16 source bytes of those four pixels start at any address (the row base is arbitrary: a pitch of 3 w + 1
// gives every row another alignment).  They are fetched as the 1, 3 or 4 (+ 1 if misaligned) ALIGNED 4-byte words that
// cover them, shifted into place in registers (gather); where they start on a word and lie wholly inside the row -- every
// interior lane of a frame whose rows start on 4 bytes -- as ONE 12- or 16-byte load.  A word is loaded only if it holds at least one byte of the row, so
// every load stays inside an aligned word that the caller's declared rows touch: no padding is asked of the caller, and the
// lanes at the ragged ends of a row read zeros for what lies outside it.
// Every offset is 64-bit.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "akz_frames.hpp"

namespace akz {
namespace {

constexpr int FT = 256;           // lanes per workgroup: 1024 output bytes of one row
constexpr uint32_t kBlocks = 8192;  // workgroups of a launch, about: 256 compute units x 8 x 4 waves, twice over; rows are looped over

struct FrameArgs {
    uint32_t w, h, n;
    uint64_t row_pitch, frame_stride, plane_stride;
};

// out[0 .. NW): the 4 NW bytes at src + off (any alignment) from aligned words; bytes outside the row [lo, hi) (offsets from
// src as well) read as 0
template <int NW>
__device__ inline void gather(const uint8_t* __restrict__ src, int64_t off, int64_t lo, int64_t hi, uint32_t (&out)[NW]) {
    const int64_t mis = (int64_t)(((uint64_t)src + (uint64_t)off) & 3);
    if (mis == 0 && off >= lo && off + 4 * NW <= hi) {  // on a word, every byte inside the row: one 4-, 12- or 16-byte load
        struct alignas(4) Words { uint32_t v[NW]; };
        const Words t = *reinterpret_cast<const Words*>(src + off);
#pragma unroll
        for (int k = 0; k < NW; ++k) out[k] = t.v[k];
        return;
    }
    const int64_t base = off - mis;
    const uint32_t shift = (uint32_t)mis * 8;
    uint32_t wd[NW + 1];
    if (base >= lo && base + 4 * (NW + 1) <= hi) {  // all NW + 1 words inside the row: unconditional loads, issued together
        struct alignas(4) Words { uint32_t v[NW + 1]; };
        const Words t = *reinterpret_cast<const Words*>(src + base);
#pragma unroll
        for (int k = 0; k <= NW; ++k) wd[k] = t.v[k];
    } else {  // the ragged ends of a row: word by word, only those that hold a byte of the row
#pragma unroll
        for (int k = 0; k <= NW; ++k) {
            const int64_t q = base + 4 * k;
            wd[k] = (q + 4 > lo && q < hi && (k < NW || shift)) ? *reinterpret_cast<const uint32_t*>(src + q) : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) out[k] = (uint32_t)((((uint64_t)wd[k + 1] << 32) | wd[k]) >> shift);
}
template <int NW>
__device__ inline uint8_t byte_of(const uint32_t (&v)[NW], int i) { return (uint8_t)(v[i >> 2] >> (8 * (i & 3))); }

template <int FMT>
__global__ void __launch_bounds__(FT) k_frame_luma(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, FrameArgs a) {
    constexpr int BPP = FMT == AKZ_FRAME_GRAY8 || FMT == AKZ_FRAME_RGB8_PLANAR ? 1 : (FMT == AKZ_FRAME_RGB8 || FMT == AKZ_FRAME_BGR8 ? 3 : 4);
    constexpr bool kSwap = FMT == AKZ_FRAME_BGR8 || FMT == AKZ_FRAME_BGRA8;
    const int64_t word = (int64_t)blockIdx.x * FT + threadIdx.x;
    for (uint32_t f = blockIdx.z; f < a.n; f += gridDim.z)
        for (uint32_t y = blockIdx.y; y < a.h; y += gridDim.y) {
            // offsets from src / dst, 64-bit: the row's first source byte and its first output byte
            const int64_t row = (int64_t)((uint64_t)f * a.frame_stride + (uint64_t)y * a.row_pitch);
            const int64_t d = (int64_t)(((uint64_t)f * a.h + y) * a.w);
            // this lane's output word holds pixels x0 .. x0 + 3 of the row (x0 < 0: the word starts in front of the row)
            const int64_t x0 = word * 4 - (int64_t)(((uint64_t)dst + (uint64_t)d) & 3);
            if (x0 >= (int64_t)a.w) continue;
            const int64_t s = row + x0 * BPP, hi = row + (int64_t)a.w * BPP;
            uint32_t l;
            if constexpr (FMT == AKZ_FRAME_GRAY8) {
                uint32_t v[1];
                gather<1>(src, s, row, hi, v);
                l = v[0];
            } else if constexpr (FMT == AKZ_FRAME_RGB8_PLANAR) {
                const int64_t ps = (int64_t)a.plane_stride;
                uint32_t r[1], g[1], b[1];
                gather<1>(src, s, row, hi, r);
                gather<1>(src, s + ps, row + ps, hi + ps, g);
                gather<1>(src, s + 2 * ps, row + 2 * ps, hi + 2 * ps, b);
                l = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) l |= (uint32_t)luma_u8(byte_of<1>(r, j), byte_of<1>(g, j), byte_of<1>(b, j)) << (8 * j);
            } else {
                uint32_t v[BPP];
                gather<BPP>(src, s, row, hi, v);
                l = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    l |= (uint32_t)luma_u8(byte_of<BPP>(v, BPP * j + (kSwap ? 2 : 0)), byte_of<BPP>(v, BPP * j + 1), byte_of<BPP>(v, BPP * j + (kSwap ? 0 : 2))) << (8 * j);
            }
            if (x0 >= 0 && x0 + 4 <= (int64_t)a.w) {
                *reinterpret_cast<uint32_t*>(dst + d + x0) = l;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j >= 0 && x0 + j < (int64_t)a.w) dst[d + x0 + j] = (uint8_t)(l >> (8 * j));
            }
        }
}

}  // namespace

namespace launch {
void frame_luma(hipStream_t s, const uint8_t* d_src, const FrameSpec& fs, uint32_t n, uint8_t* d_luma) {
    if (!fs.w || !fs.h || !n) return;
    const FrameArgs a{fs.w, fs.h, n, fs.row_pitch, fs.frame_stride, fs.plane_stride};
    // words of a row: at most three bytes of the first word lie in front of it
    const uint32_t gx = (uint32_t)((((uint64_t)fs.w + 6) / 4 + FT - 1) / FT);
    const uint32_t gz = std::min<uint32_t>(n, 65535u);
    const uint32_t gy = std::min<uint32_t>(fs.h, std::max<uint32_t>(1u, kBlocks / (uint32_t)std::min<uint64_t>((uint64_t)gx * gz, kBlocks)));
    const dim3 grid(gx, gy, gz), block(FT);
    switch (fs.format) {
        case AKZ_FRAME_GRAY8: hipLaunchKernelGGL(k_frame_luma<AKZ_FRAME_GRAY8>, grid, block, 0, s, d_src, d_luma, a); break;
        case AKZ_FRAME_RGB8: hipLaunchKernelGGL(k_frame_luma<AKZ_FRAME_RGB8>, grid, block, 0, s, d_src, d_luma, a); break;
        case AKZ_FRAME_BGR8: hipLaunchKernelGGL(k_frame_luma<AKZ_FRAME_BGR8>, grid, block, 0, s, d_src, d_luma, a); break;
        case AKZ_FRAME_RGBA8: hipLaunchKernelGGL(k_frame_luma<AKZ_FRAME_RGBA8>, grid, block, 0, s, d_src, d_luma, a); break;
        case AKZ_FRAME_BGRA8: hipLaunchKernelGGL(k_frame_luma<AKZ_FRAME_BGRA8>, grid, block, 0, s, d_src, d_luma, a); break;
        case AKZ_FRAME_RGB8_PLANAR: hipLaunchKernelGGL(k_frame_luma<AKZ_FRAME_RGB8_PLANAR>, grid, block, 0, s, d_src, d_luma, a); break;
        default: break;  // (frames_resolve refuses any other value)
    }
}
}  // namespace launch
}  // namespace akz
