// The device skeleton of every RANSAC kernel (akz_ransac_kernels.hip, akz_homography_refit.hip, akz_resection.hip; included by
// .hip files only): the matrix in LDS, one Jacobi sweep level by level on four lanes, the quad exchange of a trial's sums, the
// 256-lane tree of the refits, the winner pick and the ordered compaction of a 256-thread workgroup.  The arithmetic is the host's source (akz_fmatrix.hpp, akz_homography.hpp); what is here only moves
// loops and reductions around it.
#pragma once
#include <hip/hip_runtime.h>

#include "akz_fmatrix.hpp"
#include "akz_homography_refit.hpp"  // kRefitLanes
#include "akz_internal.hpp"

namespace akz {

constexpr int kGroup = 256;  // threads of a pick / filter or refit workgroup

// a ROWS x COLS matrix in LDS (M of akz_fmatrix.hpp); nine columns for every model of two views
template <int COLS>
struct LdsMatT {
    double* p;
    __device__ double& at(int r, int k) { return p[r * COLS + k]; }
};
using LdsMat = LdsMatT<9>;

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
// More than nine rows (the resection's twelve: 21 levels, the five widest of five or six pairs): a lane takes the level's pairs
// sub, sub + 4 one after the other -- they share no row either, so the barrier stays one per level.
template <int ROWS, int COLS = 9>
__device__ inline bool jacobi_sweep_levels(LdsMatT<COLS> m, int sub, bool active) {
    constexpr int PASSES = (ROWS / 2 + 3) / 4;  // pairs of the widest level over four lanes
    bool rotated = false;
    for (int sum = 1; sum <= 2 * ROWS - 3; ++sum) {
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {
            const int p = max(0, sum - (ROWS - 1)) + sub + 4 * pass, q = sum - p;
            if (active && p < q) rotated = jacobi_pair<COLS>(m, p, q) || rotated;
        }
        wave_sync();
    }
    return rotated;
}

// The four parts of a sum of eight (sum8_part of akz_fmatrix_normalised.hpp, one on each lane of a trial's four) combined in the
// order of sum8_join by two exchanges inside the quad: IEEE addition commutes, so all four lanes end with the bits of the host's
// sum.  (DPP quad permutes, register to register: __shfl_xor would send every sum of pass 3 through the LDS crossbar.)
template <int QUAD_PERM>
__device__ inline double quad_permute(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, QUAD_PERM, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(lo, lo, QUAD_PERM, 0xf, 0xf, false));
}
template <int N>
__device__ inline void quad_join(double (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        v[k] = v[k] + quad_permute<0x4e>(v[k]);  // lane ^ 2 (quad_perm [2, 3, 0, 1]): lanes 0, 2: p0 + p2; lanes 1, 3: p1 + p3
        v[k] = v[k] + quad_permute<0xb1>(v[k]);  // lane ^ 1 (quad_perm [1, 0, 3, 2]): (p0 + p2) + (p1 + p3)
    }
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

// One 256-wide step of the compaction in list order: the place of thread tid's element if `kept` -- written + the kept ones of
// lower threads --; written grows by the step's total on every thread.  s_wsum: kGroup / 64 counters.
__device__ inline unsigned long long compact_slot(bool kept, unsigned long long& written, unsigned* s_wsum, unsigned tid) {
    const unsigned lane = tid & 63u, w = tid >> 6;
    const unsigned long long bal = __ballot(kept);
    if (lane == 0) s_wsum[w] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (unsigned k = 0; k < kGroup / 64; ++k) {
        if (k < w) before += s_wsum[k];
        total += s_wsum[k];
    }
    const unsigned long long at = written + before;
    written += total;
    __syncthreads();
    return at;
}
// The sums of every thread's v[k] in the order of the refit's statement (akz_homography_refit.hpp; a workgroup of kRefitLanes
// threads, thread l holding lane l's sum): p[l] = p[l] + p[l + s] for s = 128, 64 through LDS, then s = 32 .. 1 inside the first
// wave with __shfl_down (lane l receives p[l] + p[l + s]; the lanes that would read past the wave never feed lane 0).  s_out[k] is
// valid for every thread on return; the caller reads it before its next call.  red: kSumGroup x 256 doubles.
constexpr int kSumGroup = 6;  // sums that go through the tree together
template <int K>
__device__ void block_sums(const double (&v)[K], double* __restrict__ red, double* __restrict__ s_out, unsigned tid) {
    constexpr int RF = kRefitLanes, RG = kSumGroup;
#pragma unroll
    for (int g = 0; g < K; g += RG) {
        double a[RG] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < RG; ++k)
            if (g + k < K) red[k * RF + tid] = v[g + k];
        __syncthreads();
        if (tid < 128) {
#pragma unroll
            for (int k = 0; k < RG; ++k)
                if (g + k < K) {
                    a[k] = red[k * RF + tid] + red[k * RF + tid + 128];
                    if (tid >= 64) red[k * RF + tid] = a[k];  // (its own slot: nobody else reads it at this level)
                }
        }
        __syncthreads();
        if (tid < 64) {
#pragma unroll
            for (int k = 0; k < RG; ++k)
                if (g + k < K) {
                    double s = a[k] + red[k * RF + tid + 64];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_down(s, o, 64);
                    if (tid == 0) s_out[g + k] = s;
                }
        }
        __syncthreads();
    }
}

// ... of a match list: thread tid's match *raw_src goes to keep_dst[its place] if `kept`
__device__ inline void compact_kept(bool kept, const akz_match* __restrict__ raw_src, akz_match* __restrict__ keep_dst,
                                    unsigned long long& written, unsigned* s_wsum, unsigned tid) {
    const unsigned long long at = compact_slot(kept, written, s_wsum, tid);
    if (kept) keep_dst[at] = *raw_src;
}

}  // namespace akz
