// k_ransac_trials: the RANSAC trials of match_features on the GPU (akaze/src/ops/estimate_fundamental_matrix.rs:99-165, called from
// akaze/src/lib.rs:267-274).  The reference runs num_trials x (8-point model + inlier count over every match) one after
// the other on one core; the host port of akz_ransac.cpp spreads the trials over host threads (1.3-1.4 ms for the 8 264
// matches of a 4K pair at 1 000 trials on 16 cores, of which 4.9 us per model in the 8 x 9 decomposition).  Here every
// trial is a workgroup: its first wave forms the model -- the same source as the host's (akz_fmatrix.hpp), f64 Jacobi
// rotations on the 8 x 9 matrix in LDS -- and the 256 threads count the inliers.  The samples are drawn on the
// host from the calling thread's random source in trial order, the winner is picked on the host in trial order with the
// reference's strict `>`, and the final filter runs on the host: same result as the host path, bit for bit.
#include <hip/hip_runtime.h>

#include "akz_fmatrix.hpp"
#include "akz_internal.hpp"

namespace akz {
namespace {

constexpr int RT = 256;

// pts: x0 | y0 | x1 | y1, n floats each; samples: 8 match indices per trial; out: per trial 9 floats (model) and the
// inlier count (-1: no model)
__global__ void __launch_bounds__(RT) k_ransac_trials(const float* __restrict__ pts, unsigned n, const unsigned* __restrict__ samples,
                                                      float epsilon_model, float epsilon_inlier, float* __restrict__ models,
                                                      int* __restrict__ inliers) {
    __shared__ float s_f[9];
    __shared__ int s_ok, s_cnt;
    __shared__ double s_m[8 * 9];
    struct LdsMat {
        double* p;
        __device__ double& at(int r, int k) { return p[r * 9 + k]; }
    };
    const unsigned trial = blockIdx.x, tid = threadIdx.x;
    const float *x0 = pts, *y0 = pts + n, *x1 = pts + 2 * (size_t)n, *y1 = pts + 3 * (size_t)n;
    // The model: the host's source (akz_fmatrix.hpp) on the matrix in LDS.  The host rotates the 28 row pairs of a sweep one
    // after the other in row-cyclic order; pairs that share no row commute, and every pair (p, q) depends only on pairs of
    // level p + q - 1 or less -- for two pairs with a common row the cyclic order and the level order agree -- so the 13
    // levels of a sweep run one after the other with the up to four pairs of a level on four lanes: the same rotations on
    // the same operands, bit for bit, along a chain of 13 instead of 28 (a rotation is ~2 000 cycles of dependent f64
    // arithmetic -- three square roots, three divisions -- and nothing else shortens a lone trial).
    if (tid < 64) {  // the workgroup's first wave; LDS operations of one wave execute in order
        LdsMat m{s_m};
        if (tid == 0) {
            float sx0[8], sy0[8], sx1[8], sy1[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned j = samples[(size_t)trial * 8 + i];
                sx0[i] = x0[j]; sy0[i] = y0[j]; sx1[i] = x1[j]; sy1[i] = y1[j];
            }
            design_matrix(m, sx0, sy0, sx1, sy1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int sweep = 0; sweep < 60; ++sweep) {
            bool rotated = false;
            for (int level = 0; level <= 12; ++level) {
                const int p = max(0, level - 6) + (int)tid, q = level + 1 - p;  // lanes 0 .. 3: the level's pairs
                if (tid < 4 && p < q) rotated = jacobi_pair(m, p, q) || rotated;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (__ballot(rotated) == 0ull) break;
        }
        if (tid == 0) {
            float f[9];
            const bool ok = model_from_rotated(m, epsilon_model, f);
            s_ok = ok ? 1 : 0;
            s_cnt = 0;
            if (ok) {
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    s_f[k] = f[k];
                    models[(size_t)trial * 9 + k] = f[k];
                }
            }
        }
    }
    __syncthreads();
    if (!s_ok) {
        if (tid == 0) inliers[trial] = -1;
        return;
    }
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = s_f[k];
    int cnt = 0;
    for (unsigned i = tid; i < n; i += RT) cnt += fundamental_error(f, x0[i], y0[i], x1[i], y1[i]) < epsilon_inlier ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63u) == 0) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0) inliers[trial] = s_cnt;
}

// ---- akz_match_features_pairs: the trials of many pairs at once ------------------------------------------------------
// A pair's matches, points, trials and kept list live at offsets the host hands over (akz_match_api.cpp: PairJobHost).
struct PairJob {
    unsigned long long raw_off, kp0_off, kp1_off, trial_off, keep_off, n_trials;
    unsigned cnt_idx, pad;
};
struct RawMatch {  // akz_match
    unsigned long long index_0, index_1;
    double distance;
};
static_assert(sizeof(PairJob) == 56 && sizeof(RawMatch) == 24, "host records");

// x0 | y0 | x1 | y1 of every match of every pair (the four arrays remove_outliers_impl builds on the host), at the pair's
// offset of the matches: a workgroup per pair (grid-stride over pairs), a thread per match
__global__ void __launch_bounds__(256) k_pair_points(const PairJob* __restrict__ pairs, unsigned n_pairs, const RawMatch* __restrict__ raw,
                                                     const unsigned long long* __restrict__ raw_cnt, const float* __restrict__ kx,
                                                     const float* __restrict__ ky, float* __restrict__ pts, unsigned long long stride) {
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const PairJob pj = pairs[p];
        const unsigned long long n = raw_cnt[pj.cnt_idx];
        for (unsigned long long i = threadIdx.x; i < n; i += blockDim.x) {
            const RawMatch m = raw[pj.raw_off + i];
            const size_t o = pj.raw_off + i, a = pj.kp0_off + m.index_0, b = pj.kp1_off + m.index_1;
            pts[o] = kx[a];
            pts[stride + o] = ky[a];
            pts[2 * stride + o] = kx[b];
            pts[3 * stride + o] = ky[b];
        }
    }
}

// k_ransac_trials for many pairs.  One trial on four lanes -- the Jacobi levels of k_ransac_trials (the same rotations on
// the same operands in the same order) -- so that a wave runs TPW trials side by side instead of one: a batch has ~10^5
// trials, and a workgroup per trial with four busy lanes held a few thousand of them on the chip.  Each trial leaves the
// sweep loop at its own first sweep without a rotation (its four lanes' ballot bits); the wave then counts the inliers of its
// trials one after the other with all 64 lanes.
constexpr int TPW = 16;  // trials per wave
constexpr int TW = 64;   // one wave per workgroup: the waves share nothing
__global__ void __launch_bounds__(TW) k_ransac_trials_multi(const PairJob* __restrict__ pairs, const unsigned* __restrict__ trials,
                                                            unsigned long long first_trial, unsigned n_trials,
                                                            const unsigned long long* __restrict__ raw_cnt, const float* __restrict__ pts,
                                                            unsigned long long stride, float epsilon_model, float epsilon_inlier,
                                                            float* __restrict__ models, int* __restrict__ inliers) {
    __shared__ double s_m[TPW][8 * 9];
    __shared__ float s_f[TPW][9];
    __shared__ int s_ok[TPW];
    struct LdsMat {
        double* p;
        __device__ double& at(int r, int k) { return p[r * 9 + k]; }
    };
    const int lane = (int)threadIdx.x, tw = lane >> 2, sub = lane & 3;
    const unsigned t0 = blockIdx.x * TPW, tl = t0 + (unsigned)tw;
    const bool valid = tl < n_trials;
    LdsMat m{s_m[tw]};
    if (valid) {  // rows sub and sub + 4 of the trial's design matrix
        const unsigned* smp = trials + (size_t)tl * 8;
        const size_t off = pairs[trials[(size_t)n_trials * 8 + tl]].raw_off;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = sub + 4 * h;
            const size_t j = off + smp[i];
            design_row(m, i, pts[j], pts[stride + j], pts[2 * stride + j], pts[3 * stride + j]);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    bool active = valid;
    for (int sweep = 0; sweep < 60; ++sweep) {
        if (__ballot(active) == 0ull) break;
        bool rotated = false;
        for (int level = 0; level <= 12; ++level) {
            const int p = max(0, level - 6) + sub, q = level + 1 - p;  // the level's pairs on the trial's four lanes
            if (active && p < q) rotated = jacobi_pair(m, p, q) || rotated;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (((__ballot(rotated) >> (4 * tw)) & 0xfull) == 0ull) active = false;  // this trial's first sweep without a rotation
    }
    if (valid && sub == 0) {
        float f[9];
        const bool ok = model_from_rotated(m, epsilon_model, f);
        const size_t t = first_trial + tl;
        s_ok[tw] = ok ? 1 : 0;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                s_f[tw][k] = f[k];
                models[t * 9 + k] = f[k];
            }
        } else {
            inliers[t] = -1;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int u = 0; u < TPW; ++u) {
        const unsigned t = t0 + (unsigned)u;
        if (t >= n_trials) break;
        if (!s_ok[u]) continue;
        const PairJob pj = pairs[trials[(size_t)n_trials * 8 + t]];
        const unsigned n = (unsigned)raw_cnt[pj.cnt_idx];
        const float *x0 = pts + pj.raw_off, *y0 = x0 + stride, *x1 = y0 + stride, *y1 = x1 + stride;
        float f[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = s_f[u][k];
        int cnt = 0;
        for (unsigned i = (unsigned)lane; i < n; i += TW) cnt += fundamental_error(f, x0[i], y0[i], x1[i], y1[i]) < epsilon_inlier ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) inliers[first_trial + t] = cnt;
    }
}

// Per pair (a workgroup, grid-stride): the winner -- the first trial with the most inliers, strict `>` from 0 in trial order
// (the largest count, the lowest trial among equals); none above 0: the zero model -- and the matches it keeps
// (fundamental_error < epsilon, as the host's final filter), compacted in match order.  Fewer than 8 matches: all kept.
constexpr int PF = 256;
__global__ void __launch_bounds__(PF) k_ransac_pick_filter(const PairJob* __restrict__ pairs, unsigned n_pairs, const RawMatch* __restrict__ raw,
                                                           const unsigned long long* __restrict__ raw_cnt, const float* __restrict__ pts,
                                                           unsigned long long stride, const float* __restrict__ models,
                                                           const int* __restrict__ inliers, float epsilon_inlier, RawMatch* __restrict__ keep,
                                                           unsigned long long* __restrict__ keep_cnt) {
    __shared__ int s_best[PF / 64];
    __shared__ unsigned long long s_idx[PF / 64];
    __shared__ unsigned s_wsum[PF / 64];
    __shared__ float s_f[9];
    const unsigned tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const PairJob pj = pairs[p];
        const unsigned long long n = raw_cnt[pj.cnt_idx];
        int best = 0;
        unsigned long long bidx = ~0ull;
        if (n >= 8)
            for (unsigned long long t = tid; t < pj.n_trials; t += PF) {
                const int v = inliers[pj.trial_off + t];
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
        if (lane == 0) {
            s_best[w] = best;
            s_idx[w] = bidx;
        }
        __syncthreads();
        if (tid == 0) {
            for (unsigned k = 1; k < PF / 64; ++k)
                if (s_best[k] > best || (s_best[k] == best && s_idx[k] < bidx)) {
                    best = s_best[k];
                    bidx = s_idx[k];
                }
            for (int k = 0; k < 9; ++k) s_f[k] = best > 0 ? models[(pj.trial_off + bidx) * 9 + k] : 0.0f;
        }
        __syncthreads();
        float f[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = s_f[k];
        const float *x0 = pts + pj.raw_off, *y0 = x0 + stride, *x1 = y0 + stride, *y1 = x1 + stride;
        unsigned long long written = 0;
        for (unsigned long long base = 0; base < n; base += PF) {
            const unsigned long long i = base + tid;
            const bool kept = i < n && (n < 8 || fundamental_error(f, x0[i], y0[i], x1[i], y1[i]) < epsilon_inlier);
            const unsigned long long bal = __ballot(kept);
            if (lane == 0) s_wsum[w] = (unsigned)__popcll(bal);
            __syncthreads();
            unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull)), total = 0;
            for (unsigned k = 0; k < PF / 64; ++k) {
                if (k < w) before += s_wsum[k];
                total += s_wsum[k];
            }
            if (kept) keep[pj.keep_off + written + before] = raw[pj.raw_off + i];
            written += total;
            __syncthreads();
        }
        if (tid == 0) keep_cnt[p] = written;
    }
}

}  // namespace

namespace launch {
void pair_points(hipStream_t s, const PairJobHost* d_pairs, uint32_t n_pairs, const void* d_raw, const uint64_t* d_raw_cnt,
                 const float* d_kx, const float* d_ky, float* d_pts, uint64_t pts_stride) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(k_pair_points, dim3(std::min<uint32_t>(n_pairs, 8192)), dim3(256), 0, s, (const PairJob*)d_pairs, n_pairs,
                       (const RawMatch*)d_raw, (const unsigned long long*)d_raw_cnt, d_kx, d_ky, d_pts, (unsigned long long)pts_stride);
}
void ransac_trials_multi(hipStream_t s, const PairJobHost* d_pairs, const uint32_t* d_trials, uint64_t first_trial, uint32_t n_trials,
                         const uint64_t* d_raw_cnt, const float* d_pts, uint64_t pts_stride, float epsilon_model, float epsilon_inlier,
                         float* d_models, int32_t* d_inliers) {
    if (n_trials == 0) return;
    hipLaunchKernelGGL(k_ransac_trials_multi, dim3((n_trials + TPW - 1) / TPW), dim3(TW), 0, s, (const PairJob*)d_pairs, d_trials,
                       (unsigned long long)first_trial, n_trials, (const unsigned long long*)d_raw_cnt, d_pts, (unsigned long long)pts_stride,
                       epsilon_model, epsilon_inlier, d_models, d_inliers);
}
void ransac_pick_filter(hipStream_t s, const PairJobHost* d_pairs, uint32_t n_pairs, const void* d_raw, const uint64_t* d_raw_cnt,
                        const float* d_pts, uint64_t pts_stride, const float* d_models, const int32_t* d_inliers, float epsilon_inlier,
                        void* d_keep, uint64_t* d_keep_cnt) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(k_ransac_pick_filter, dim3(std::min<uint32_t>(n_pairs, 8192)), dim3(PF), 0, s, (const PairJob*)d_pairs, n_pairs,
                       (const RawMatch*)d_raw, (const unsigned long long*)d_raw_cnt, d_pts, (unsigned long long)pts_stride, d_models,
                       d_inliers, epsilon_inlier, (RawMatch*)d_keep, (unsigned long long*)d_keep_cnt);
}
void ransac_trials(hipStream_t s, const float* d_pts, uint32_t n_matches, const uint32_t* d_samples, uint32_t trials, float epsilon_model,
                   float epsilon_inlier, float* d_models, int32_t* d_inliers) {
    if (trials == 0) return;
    hipLaunchKernelGGL(k_ransac_trials, dim3(trials), dim3(RT), 0, s, d_pts, n_matches, d_samples, epsilon_model, epsilon_inlier, d_models,
                       d_inliers);
}
}  // namespace launch
}  // namespace akz
