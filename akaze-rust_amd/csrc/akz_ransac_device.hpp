// The device skeleton of every RANSAC kernel (akz_ransac_kernels.hip, akz_homography_refit.hip, akz_resection.hip; included by
// .hip files only): the matrix in LDS, one Jacobi sweep level by level on four lanes, the quad exchange of a trial's sums, the
// 256-lane tree of the refits, the winner pick, the ordered compaction of a 256-thread workgroup, and refit_loop with block_count:
// the refit loop of every model (the statement and the refit concept: akz_homography_refit.hpp).  The arithmetic is the host's
// source (akz_fmatrix.hpp, akz_homography.hpp, akz_resection.hpp); what is here only moves loops and reductions around it.
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

// One pair's points as every model of two views reads them, and the pairs calls' table that yields it: x0 | y0 | x1 | y1 at the
// pair's offset of the matches (k_pair_points), the count of its raw list
struct PairView {
    const float *x0, *y0, *x1, *y1;
    unsigned n;
};
struct PairTable {
    const launch::PairJobHost* pairs;
    const unsigned long long* raw_cnt;
    const float* pts;
    unsigned long long stride;
    __device__ PairView view(unsigned p) const {
        const launch::PairJobHost pj = pairs[p];
        const float* x0 = pts + pj.raw_off;
        return PairView{x0, x0 + stride, x0 + 2 * stride, x0 + 3 * stride, (unsigned)raw_cnt[pj.cnt_idx]};
    }
};

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

// |{ i < v.n : inlier under h }| for every thread of the 256
template <class R, class View>
__device__ unsigned block_count(const float (&h)[R::kFloats], const View& v, float eps, unsigned* s_wsum, unsigned tid) {
    unsigned cnt = 0;
    for (unsigned i = tid; i < v.n; i += kGroup) cnt += R::inlier(h, v, i, eps) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63u) == 0) s_wsum[tid >> 6] = cnt;
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int k = 0; k < kGroup / 64; ++k) total += s_wsum[k];
    __syncthreads();
    return total;
}

// The loop of the refit's statement (akz_homography_refit.hpp) for the refit model R over the view v, by a workgroup of 256 and the
// same for all its threads: h is the model to start from and the last accepted one on return; -> the fits accepted.  Element i is
// thread i mod 256's, added in ascending i: the lane sums live in f64 registers and go through the tree six at a time
// (block_sums).  M stays in LDS, as the trial wave keeps its own: its rotations run on four lanes of the first wave
// (jacobi_sweep_levels); the smallest row, the rank rule and the model tail on thread 0.  The caller passes a __syncthreads before
// the next call (s_ok, s_h, s_sum).  s_wsum: kGroup / 64 counters, the caller's (its compaction uses them too).
// (The compiler simplifies this function on its own before it inlines it, and the two-view kernels sit at 256 registers: the view by
// value and the model in a local array keep both out of memory that the LDS stores might alias there; `static` keeps the LDS arrays
// laid out as a kernel's own.  Without either an instance spills or pads its LDS.)
template <class R, class View>
static __device__ __forceinline__ unsigned refit_loop(const View v, float (&h_io)[R::kFloats], float epsilon_model, float epsilon_inlier,
                                                      unsigned max_iterations, unsigned* s_wsum, unsigned tid) {
    static_assert(kRefitLanes == kGroup, "block_sums");
    constexpr int MF = R::kFloats, S1 = R::kSums1, S3 = R::kSums3, ROWS = R::kRows;
    __shared__ double s_red[kSumGroup * kGroup];
    __shared__ double s_sum[S3];
    __shared__ double s_m[ROWS * ROWS];
    __shared__ float s_h[MF];
    __shared__ int s_ok;
    float h[MF];
#pragma unroll
    for (int k = 0; k < MF; ++k) h[k] = h_io[k];
    unsigned cnt = block_count<R>(h, v, epsilon_inlier, s_wsum, tid);
    unsigned done = 0;
    while (done < max_iterations) {
        if (cnt < (unsigned)R::kMin) break;
        const double count = (double)cnt;
        double c[S1], s0 = 0.0, s1 = 0.0;
        {
            double a[S1];
#pragma unroll
            for (int k = 0; k < S1; ++k) a[k] = 0.0;
            for (unsigned i = tid; i < v.n; i += kGroup)
                if (R::inlier(h, v, i, epsilon_inlier)) {
                    double t[S1];
                    R::terms1(v, i, t);
#pragma unroll
                    for (int k = 0; k < S1; ++k) a[k] = a[k] + t[k];
                }
            block_sums<S1>(a, s_red, s_sum, tid);
#pragma unroll
            for (int k = 0; k < S1; ++k) c[k] = s_sum[k] / count;
        }
        {
            double a[2] = {0.0, 0.0};
            for (unsigned i = tid; i < v.n; i += kGroup)
                if (R::inlier(h, v, i, epsilon_inlier)) {
                    double t[2];
                    R::terms2(v, i, c, t);
                    a[0] = a[0] + t[0];
                    a[1] = a[1] + t[1];
                }
            block_sums<2>(a, s_red, s_sum, tid);
            const double d0 = s_sum[0], d1 = s_sum[1];
            if (!refit_scale(d0, count, s0) || !R::scale2(d1, count, s1)) break;  // (the same for every thread)
        }
        {
            double a[S3];
#pragma unroll
            for (int k = 0; k < S3; ++k) a[k] = 0.0;
            for (unsigned i = tid; i < v.n; i += kGroup)
                if (R::inlier(h, v, i, epsilon_inlier)) {
                    double t[S3];
                    R::terms3(v, i, c, s0, s1, t);
#pragma unroll
                    for (int k = 0; k < S3; ++k) a[k] = a[k] + t[k];
                }
            block_sums<S3>(a, s_red, s_sum, tid);
        }
        if (tid < 64) {  // the first wave: M, the sweeps on its lanes 0 .. 3, the model on lane 0
            LdsMatT<ROWS> m{s_m};
            if (tid == 0) R::normal_matrix(m, s_sum);
            wave_sync();
            for (int sweep = 0; sweep < 60; ++sweep)
                if (__ballot(jacobi_sweep_levels<ROWS, ROWS>(m, (int)tid, tid < 4)) == 0ull) break;  // the first sweep without a rotation
            if (tid == 0) {
                float h2[MF];
                const bool ok = R::model_from_rotated(m, count, epsilon_model, c, s0, s1, h2);
                s_ok = ok ? 1 : 0;
                if (ok) {
#pragma unroll
                    for (int k = 0; k < MF; ++k) s_h[k] = h2[k];
                }
            }
        }
        __syncthreads();
        if (s_ok == 0) break;
        float h2[MF];
#pragma unroll
        for (int k = 0; k < MF; ++k) h2[k] = s_h[k];
        const unsigned cnt2 = block_count<R>(h2, v, epsilon_inlier, s_wsum, tid);
        if (cnt2 < cnt) break;  // h2 is rejected
        const bool grew = cnt2 > cnt;
#pragma unroll
        for (int k = 0; k < MF; ++k) h[k] = h2[k];
        cnt = cnt2;
        ++done;
        if (!grew) break;
    }
#pragma unroll
    for (int k = 0; k < MF; ++k) h_io[k] = h[k];
    return done;
}

// ... of a match list: thread tid's match *raw_src goes to keep_dst[its place] if `kept`
__device__ inline void compact_kept(bool kept, const akz_match* __restrict__ raw_src, akz_match* __restrict__ keep_dst,
                                    unsigned long long& written, unsigned* s_wsum, unsigned tid) {
    const unsigned long long at = compact_slot(kept, written, s_wsum, tid);
    if (kept) keep_dst[at] = *raw_src;
}

}  // namespace akz
