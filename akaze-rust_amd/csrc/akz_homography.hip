// The homography RANSAC of akz_match_features_homography(_pairs) on the GPU: the model source of the host path
// (akz_homography.hpp), the trial layout of k_ransac_trials_multi (akz_fmatrix.hip) and the pair records of
// akz_match_features_pairs (PairJobHost: a pair's matches, points, trials and kept list at offsets the host hands over).
// Samples are drawn on the host, 4 per trial; everything else -- models, inlier counts, the winner, H and the kept lists --
// is formed here, bit for bit what akz_remove_outliers_homography forms on the host.
#include <hip/hip_runtime.h>

#include "akz_homography.hpp"
#include "akz_internal.hpp"

namespace akz {
namespace {

using PairJob = launch::PairJobHost;

// TPW trials per wave, four lanes per trial.  Each lane loads the whole 4-point sample and forms its normalisation and
// degeneracy test itself (the same operands in the same order: the same bits on all four), then writes the two design rows
// of its own correspondence into the trial's LDS matrix.  The 13 Jacobi levels run on the trial's four lanes (the rotations
// of the host's row-cyclic sweep, see k_ransac_trials), each trial leaving at its own first sweep without a rotation; the
// null-vector projection and the denormalisation run on one lane per trial; the wave then counts the inliers of its trials
// one after the other with all 64 lanes.  Output per trial: the model (9 floats) and the inlier count, or -1 (no model).
// NW > 1: the workgroup has NW - 1 more waves that only help count (a launch of few trials -- one pair, 1 000 trials, is 63
// waves -- leaves most of the chip idle while each wave counts 16 trials over every match: single calls on 4K pairs took
// 1.8x the fundamental-matrix call's time with one wave).  Counts are integers: the same for every NW.
constexpr int TPW = 16;
constexpr int TW = 64;
template <int NW>
__global__ void __launch_bounds__(TW * NW) k_homography_trials(const PairJob* __restrict__ pairs, const unsigned* __restrict__ trials,
                                                          unsigned long long first_trial, unsigned n_trials,
                                                          const unsigned long long* __restrict__ raw_cnt, const float* __restrict__ pts,
                                                          unsigned long long stride, float epsilon_model, float epsilon_inlier,
                                                          float* __restrict__ models, int* __restrict__ inliers) {
    __shared__ double s_m[TPW][8 * 9];
    __shared__ double s_t[TPW][6];  // c0x, c0y, s0, c1x, c1y, s1
    __shared__ float s_h[TPW][9];
    __shared__ int s_ok[TPW];
    __shared__ int s_cnt[TPW];
    struct LdsMat {
        double* p;
        __device__ double& at(int r, int k) { return p[r * 9 + k]; }
    };
    const int tid = (int)threadIdx.x, lane = tid & (TW - 1), tw = lane >> 2, sub = lane & 3;
    const unsigned t0 = blockIdx.x * TPW, tl = t0 + (unsigned)tw;
    if (tid < TW) {  // the models: the first wave
        const bool valid = tl < n_trials;
        LdsMat m{s_m[tw]};
        bool sample_ok = false;
        if (valid) {
            const unsigned* smp = trials + (size_t)tl * 4;
            const size_t off = pairs[trials[(size_t)n_trials * 4 + tl]].raw_off;
            float x0[4], y0[4], x1[4], y1[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t j = off + smp[i];
                x0[i] = pts[j]; y0[i] = pts[stride + j]; x1[i] = pts[2 * stride + j]; y1[i] = pts[3 * stride + j];
            }
            HomSample hs;
            sample_ok = hom_prepare(x0, y0, x1, y1, hs);
            if (sample_ok) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i == sub) hom_rows(m, i, hs.x0[i], hs.y0[i], hs.x1[i], hs.y1[i]);
                if (sub == 0) {
                    s_t[tw][0] = hs.c0x; s_t[tw][1] = hs.c0y; s_t[tw][2] = hs.s0;
                    s_t[tw][3] = hs.c1x; s_t[tw][4] = hs.c1y; s_t[tw][5] = hs.s1;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        bool active = sample_ok;
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
            float h[9];
            const bool ok = sample_ok && hom_model_from_rotated(m, epsilon_model, s_t[tw][0], s_t[tw][1], s_t[tw][2], s_t[tw][3], s_t[tw][4],
                                                                s_t[tw][5], h);
            const size_t t = first_trial + tl;
            s_ok[tw] = ok ? 1 : 0;
            s_cnt[tw] = 0;
            if (ok) {
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    s_h[tw][k] = h[k];
                    models[t * 9 + k] = h[k];
                }
            } else {
                inliers[t] = -1;
            }
        }
    }
    __syncthreads();
    for (int u = 0; u < TPW; ++u) {
        const unsigned t = t0 + (unsigned)u;
        if (t >= n_trials) break;
        if (!s_ok[u]) continue;
        const PairJob pj = pairs[trials[(size_t)n_trials * 4 + t]];
        const unsigned n = (unsigned)raw_cnt[pj.cnt_idx];
        const float *x0 = pts + pj.raw_off, *y0 = x0 + stride, *x1 = y0 + stride, *y1 = x1 + stride;
        float h[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) h[k] = s_h[u][k];
        int cnt = 0;
        for (unsigned i = (unsigned)tid; i < n; i += TW * NW) cnt += homography_inlier(h, x0[i], y0[i], x1[i], y1[i], epsilon_inlier) ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (NW == 1) {
            if (lane == 0) inliers[first_trial + t] = cnt;
        } else if (lane == 0) {
            atomicAdd(&s_cnt[u], cnt);
        }
    }
    if (NW > 1) {
        __syncthreads();
        if (tid < TPW && t0 + (unsigned)tid < n_trials && s_ok[tid]) inliers[first_trial + t0 + tid] = s_cnt[tid];
    }
}

// Per pair (a workgroup, grid-stride): the winner -- the first trial with the most inliers, strict `>` from 0 in trial order
// --, its H and found = 1, and the matches it keeps compacted in match order; no trial above 0 (or fewer than 4 matches):
// every match kept, found = 0, H left as zeros.
constexpr int PF = 256;
__global__ void __launch_bounds__(PF) k_homography_pick_filter(const PairJob* __restrict__ pairs, unsigned n_pairs,
                                                               const akz_match* __restrict__ raw, const unsigned long long* __restrict__ raw_cnt,
                                                               const float* __restrict__ pts, unsigned long long stride,
                                                               const float* __restrict__ models, const int* __restrict__ inliers,
                                                               float epsilon_inlier, akz_match* __restrict__ keep,
                                                               unsigned long long* __restrict__ keep_cnt, float* __restrict__ h_out,
                                                               int* __restrict__ found_out) {
    __shared__ int s_best[PF / 64];
    __shared__ unsigned long long s_idx[PF / 64];
    __shared__ unsigned s_wsum[PF / 64];
    __shared__ float s_h[9];
    __shared__ int s_found;
    const unsigned tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const PairJob pj = pairs[p];
        const unsigned long long n = raw_cnt[pj.cnt_idx];
        int best = 0;
        unsigned long long bidx = ~0ull;
        if (n >= 4)
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
            s_found = best > 0 ? 1 : 0;
            for (int k = 0; k < 9; ++k) {
                s_h[k] = best > 0 ? models[(pj.trial_off + bidx) * 9 + k] : 0.0f;
                h_out[(size_t)p * 9 + k] = s_h[k];
            }
            found_out[p] = s_found;
        }
        __syncthreads();
        const bool all = s_found == 0;
        float h[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) h[k] = s_h[k];
        const float *x0 = pts + pj.raw_off, *y0 = x0 + stride, *x1 = y0 + stride, *y1 = x1 + stride;
        unsigned long long written = 0;
        for (unsigned long long base = 0; base < n; base += PF) {
            const unsigned long long i = base + tid;
            const bool kept = i < n && (all || homography_inlier(h, x0[i], y0[i], x1[i], y1[i], epsilon_inlier));
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
void homography_trials(hipStream_t s, const PairJobHost* d_pairs, const uint32_t* d_trials, uint64_t first_trial, uint32_t n_trials,
                       const uint64_t* d_raw_cnt, const float* d_pts, uint64_t pts_stride, float epsilon_model, float epsilon_inlier,
                       float* d_models, int32_t* d_inliers) {
    if (n_trials == 0) return;
    // fewer workgroups than half the chip's SIMDs (256 CUs x 4): three helper waves per workgroup for the counts
    const uint32_t blocks = (n_trials + TPW - 1) / TPW;
    if (blocks < 512)
        hipLaunchKernelGGL(k_homography_trials<4>, dim3(blocks), dim3(TW * 4), 0, s, d_pairs, d_trials, (unsigned long long)first_trial,
                           n_trials, (const unsigned long long*)d_raw_cnt, d_pts, (unsigned long long)pts_stride, epsilon_model,
                           epsilon_inlier, d_models, d_inliers);
    else
        hipLaunchKernelGGL(k_homography_trials<1>, dim3(blocks), dim3(TW), 0, s, d_pairs, d_trials, (unsigned long long)first_trial,
                           n_trials, (const unsigned long long*)d_raw_cnt, d_pts, (unsigned long long)pts_stride, epsilon_model,
                           epsilon_inlier, d_models, d_inliers);
}
void homography_pick_filter(hipStream_t s, const PairJobHost* d_pairs, uint32_t n_pairs, const void* d_raw, const uint64_t* d_raw_cnt,
                            const float* d_pts, uint64_t pts_stride, const float* d_models, const int32_t* d_inliers, float epsilon_inlier,
                            void* d_keep, uint64_t* d_keep_cnt, float* d_h, int32_t* d_found) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(k_homography_pick_filter, dim3(std::min<uint32_t>(n_pairs, 8192)), dim3(PF), 0, s, d_pairs, n_pairs,
                       (const akz_match*)d_raw, (const unsigned long long*)d_raw_cnt, d_pts, (unsigned long long)pts_stride, d_models,
                       d_inliers, epsilon_inlier, (akz_match*)d_keep, (unsigned long long*)d_keep_cnt, d_h, d_found);
}
}  // namespace launch
}  // namespace akz
