// k_mask_candidates: the detection mask of an extraction, as a compaction of the job's unordered NMS candidate list.
//
// A candidate of level l (octave o, r = 1 << o) at level pixel (x, y) stays only if
//     mask[img][(y << o) + (r >> 1)][(x << o) + (r >> 1)] != 0
// -- the rounded position the reference gives the unrefined keypoint (x r + 0.5 (r - 1), scale_space_extrema.rs:89-92), which lies
// inside the frame because the level is W >> o wide.  The pyramid and every plane are untouched; a candidate that goes never reaches
// the sorts, k_relations, k_select or the host's cache walk, exactly like one the border test removes (nms_emit).
//
// Shape.  One thread per candidate, a grid-stride loop over min(count, cap) records of 32 bytes, walked twice by at most kMaskBlocks
// workgroups.  The list is an atomic append whose order nothing relies on (it is sorted afterwards on the unique key image, level,
// index), so the kept records are appended to a SECOND buffer through one counter: a workgroup first COUNTS what it keeps (the
// per-lane atomicAdd on one LDS word is folded into one per wave by the compiler), reserves its range with ONE global atomic, then
// walks its records again and stores the kept ones there.  (One global atomic per wave and walk, as first built: 1 150 atomics on one
// address for the 74 000 candidates of a 32-frame 1080p batch, 0.11 ms per launch; profiles/r27_extract_mask.json has both.)
// Nothing is compacted in place across workgroups.
// Count words (cnt, 4 x u32, 8-byte aligned).  On entry cnt[0] is the list's length; cnt[2] (kept so far) and cnt[3] (workgroups
// done) are zero (launch::mask_candidates clears cnt[1 .. 3] on the stream in front of the launch) and are advanced TOGETHER, as one
// 64-bit word: a workgroup's atomic adds its kept count to the low half and 1 to the high half, and what it returns is the
// workgroup's first output index and its ticket.  Every workgroup reads cnt[0] before that atomic, and the workgroup that takes the
// last ticket -- it then knows the total -- stores cnt[1] = the length on entry, cnt[0] = the kept count and clears cnt[2], cnt[3].
// Overflow.  cnt[0] > cap: the list is truncated and the finish half redoes the extrema with room.  The first cap records are then
// copied through unfiltered, so the consumers that run before the host has seen the count find the list they would find without
// a mask, and cnt[0] stays as it is for the existing overflow path; cnt[1] = cnt[0].
// Bounds.  A record whose level, image or index lies outside the job's tables is dropped without a mask read: no address is
// formed from it.  Every offset is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "akz_internal.hpp"

namespace akz {
namespace {

constexpr int MT = 256;                 // lanes per workgroup
constexpr uint32_t kMaskBlocks = 128;  // workgroups of a launch at most (the loop strides over longer lists): as many atomics on the one counter

struct MaskArgs {
    const uint8_t* mask;
    uint64_t row_pitch, frame_stride;  // bytes; frame_stride 0: one mask for every image
    uint32_t n_images, n_levels;
    uint32_t lw[kMaxLevels], lh[kMaxLevels];
    uint8_t octave[kMaxLevels];
};

// does the mask let this record through?  (a record outside the job's tables: no, and no address is formed from it)
__device__ inline bool mask_keeps(const Candidate& c, const MaskArgs& a, const uint32_t* s_w, const uint32_t* s_h, const uint32_t* s_o) {
    if (c.level >= a.n_levels || c.img >= a.n_images) return false;
    const uint32_t w = s_w[c.level], h = s_h[c.level], o = s_o[c.level];
    const uint32_t y = c.idx / w, x = c.idx - y * w;
    if (y >= h) return false;
    const uint32_t half = (1u << o) >> 1;
    const uint64_t my = ((uint64_t)y << o) + half, mx = ((uint64_t)x << o) + half;
    return a.mask[(uint64_t)c.img * a.frame_stride + my * a.row_pitch + mx] != 0;
}

__global__ void __launch_bounds__(MT) k_mask_candidates(const Candidate* __restrict__ in, Candidate* __restrict__ out, uint32_t cap,
                                                         uint32_t* __restrict__ cnt, MaskArgs a) {
    // the level tables by a lane's own index: from LDS, not by a per-lane load from the kernel arguments
    __shared__ uint32_t s_w[kMaxLevels], s_h[kMaxLevels], s_o[kMaxLevels];
    __shared__ uint32_t s_kept, s_at, s_base, s_last;
    const uint32_t tid = threadIdx.x;
    if (tid < (uint32_t)kMaxLevels) {
        s_w[tid] = a.lw[tid];
        s_h[tid] = a.lh[tid];
        s_o[tid] = a.octave[tid];
    }
    if (tid == 0) s_kept = 0, s_at = 0;
    __syncthreads();
    const uint32_t entry = cnt[0];
    const bool overflow = entry > cap;
    const uint32_t m = overflow ? cap : entry;
    const uint32_t first = blockIdx.x * MT + tid, step = gridDim.x * MT;
    // 1. count (an overflowed list is copied through: nothing to count)
    uint32_t mine = 0;
    if (!overflow)
        for (uint32_t i = first; i < m; i += step) mine += mask_keeps(in[i], a, s_w, s_h, s_o) ? 1u : 0u;
    if (mine) atomicAdd(&s_kept, mine);
    __syncthreads();
    // 2. reserve: kept count and ticket in one atomic
    if (tid == 0) {
        const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long*>(cnt + 2), (unsigned long long)s_kept | (1ull << 32));
        s_base = (uint32_t)old;
        s_last = (uint32_t)(old >> 32) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    // 3. store (s_base + s_kept <= m <= cap: at most m records are kept over all workgroups)
    for (uint32_t i = first; i < m; i += step) {
        const Candidate c = in[i];
        if (overflow) {
            out[i] = c;
        } else if (mask_keeps(c, a, s_w, s_h, s_o)) {
            const uint32_t k = atomicAdd(&s_at, 1u);
            if (k < s_kept) out[s_base + k] = c;  // (always, unless the caller changed the mask between the two walks: never past the reserved range)
        }
    }
    // the workgroup with the last ticket publishes the counts: every other one has read cnt[0] and added its share
    if (s_last && tid == 0) {
        cnt[1] = entry;
        if (!overflow) cnt[0] = s_base + s_kept;
        cnt[2] = 0;
        cnt[3] = 0;
    }
}

}  // namespace

namespace launch {
void mask_candidates(hipStream_t s, const Candidate* d_in, Candidate* d_out, uint32_t cap, uint32_t* d_cnt, const uint8_t* d_mask,
                     uint64_t row_pitch, uint64_t frame_stride, const uint32_t* level_w, const uint32_t* level_h,
                     const uint32_t* level_octave, uint32_t n_levels, uint32_t n_images) {
    MaskArgs a{};
    a.mask = d_mask, a.row_pitch = row_pitch, a.frame_stride = frame_stride;
    a.n_images = n_images, a.n_levels = std::min<uint32_t>(n_levels, (uint32_t)kMaxLevels);
    for (uint32_t l = 0; l < (uint32_t)kMaxLevels; ++l) {
        const bool in = l < a.n_levels;
        a.lw[l] = in ? std::max<uint32_t>(level_w[l], 1u) : 1u;
        a.lh[l] = in ? level_h[l] : 0u;
        a.octave[l] = in ? (uint8_t)std::min<uint32_t>(level_octave[l], 31u) : 0;
    }
    (void)hipMemsetAsync(d_cnt + 1, 0, 3 * sizeof(uint32_t), s);
    const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>(kMaskBlocks, (cap + MT - 1) / MT));
    hipLaunchKernelGGL(k_mask_candidates, dim3(blocks), dim3(MT), 0, s, d_in, d_out, cap, d_cnt, a);
}
}  // namespace launch
}  // namespace akz
