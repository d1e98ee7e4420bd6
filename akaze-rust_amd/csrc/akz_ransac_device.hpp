// The device skeleton of every RANSAC kernel (akz_ransac_kernels.hip, akz_homography_refit.hip; included by .hip files only):
// the matrix in LDS, one Jacobi sweep level by level on four lanes, the winner pick and the ordered compaction of a
// 256-thread workgroup.  The arithmetic is the host's source (akz_fmatrix.hpp, akz_homography.hpp); what is here only moves
// loops and reductions around it.
#pragma once
#include <hip/hip_runtime.h>

#include "akz_fmatrix.hpp"
#include "akz_internal.hpp"

namespace akz {

constexpr int kGroup = 256;  // threads of a pick / filter or refit workgroup

// a ROWS x 9 matrix in LDS (M of akz_fmatrix.hpp)
struct LdsMat {
    double* p;
    __device__ double& at(int r, int k) { return p[r * 9 + k]; }
};

// LDS operations of one wave execute in order; this makes the lanes' writes visible to each other
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ONE sweep of the host's jacobi_sweeps_rows<ROWS> on four lanes (sub = 0 .. 3 of an active group); true: this lane rotated.
// The host rotates the pairs (0,1) (0,2) .. (ROWS-2,ROWS-1) one after the other in row-cyclic order.  Pairs that share no row
// commute, the pairs of one level p + q = sum touch disjoint rows, and every pair of the cyclic order that shares a row with
// (p, q) and comes before it has a smaller sum, every later one a larger.  So the 2 ROWS - 3 levels run one after the other
// with the up to four pairs of a level on four lanes: the same rotations on the same operands, bit for bit, along a chain of
// 13 (15 for nine rows) instead of 28 (36) -- a rotation is ~2 000 cycles of dependent f64 arithmetic, three square roots,
// three divisions, and nothing else shortens a lone decomposition.
// Every lane of the wave calls this (the barrier is the wave's): `active` masks the rotations, it does not branch around the
// call.  When to stop sweeping is the caller's: the whole wave or each group of four at its first sweep without a rotation.
template <int ROWS>
__device__ inline bool jacobi_sweep_levels(LdsMat m, int sub, bool active) {
    bool rotated = false;
    for (int sum = 1; sum <= 2 * ROWS - 3; ++sum) {
        const int p = max(0, sum - (ROWS - 1)) + sub, q = sum - p;
        if (active && p < q) rotated = jacobi_pair(m, p, q) || rotated;
        wave_sync();
    }
    return rotated;
}

// The winner among trials trial_off .. + n_trials of a 256-thread workgroup: the first trial with the most inliers, strict `>`
// from 0 in trial order (the largest count, the lowest trial among equals); best = 0: none.  Valid on thread 0 only;
// `enabled` is the same for the whole workgroup, which passes one __syncthreads.
struct Winner {
    int best;
    unsigned long long bidx;
};
__device__ inline Winner pick_winner(const int* __restrict__ inliers, unsigned long long trial_off, unsigned long long n_trials, bool enabled,
                                     int* s_best, unsigned long long* s_idx, unsigned tid) {
    int best = 0;
    unsigned long long bidx = ~0ull;
    if (enabled)
        for (unsigned long long t = tid; t < n_trials; t += kGroup) {
            const int v = inliers[trial_off + t];
            if (v > best) {
                best = v;
                bidx = t;
            }
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_xor(best, o, 64);
        const unsigned long long oi = __shfl_xor(bidx, o, 64);
        if (ob > best || (ob == best && oi < bidx)) {
            best = ob;
            bidx = oi;
        }
    }
    if ((tid & 63u) == 0) {
        s_best[tid >> 6] = best;
        s_idx[tid >> 6] = bidx;
    }
    __syncthreads();
    if (tid == 0)
        for (unsigned k = 1; k < kGroup / 64; ++k)
            if (s_best[k] > best || (s_best[k] == best && s_idx[k] < bidx)) {
                best = s_best[k];
                bidx = s_idx[k];
            }
    return Winner{best, bidx};
}

// One 256-wide step of the compaction in match order: thread tid's match *raw_src goes to keep_dst[written + the kept ones of
// lower threads] if `kept`; written grows by the step's total on every thread.  s_wsum: kGroup / 64 counters.
__device__ inline void compact_kept(bool kept, const akz_match* __restrict__ raw_src, akz_match* __restrict__ keep_dst,
                                    unsigned long long& written, unsigned* s_wsum, unsigned tid) {
    const unsigned lane = tid & 63u, w = tid >> 6;
    const unsigned long long bal = __ballot(kept);
    if (lane == 0) s_wsum[w] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (unsigned k = 0; k < kGroup / 64; ++k) {
        if (k < w) before += s_wsum[k];
        total += s_wsum[k];
    }
    if (kept) keep_dst[written + before] = *raw_src;
    written += total;
    __syncthreads();
}

}  // namespace akz
