// The RANSAC of match_features on the GPU, for both models (akaze/src/ops/estimate_fundamental_matrix.rs:99-165, called from
// akaze/src/lib.rs:267-274; the homography is an addition).  The reference runs num_trials x (model of a sample +
// inlier count over every match) one after the other on one core; the host port of akz_ransac.cpp spreads the trials over
// host threads.  Here the models come from the host's source (akz_fmatrix.hpp, akz_homography.hpp: f64 Jacobi rotations on
// the 8 x 9 matrix, in LDS) through the one skeleton of akz_ransac_device.hpp.  Samples are always drawn on the host from the
// calling thread's random source in trial order; what is formed here has the bits of the host path.
//   k_ransac_trials                       akz_match_features: a workgroup per trial of one pair, winner and filter on the host
//   k_pair_points, k_pairs_trials<Model, NW>, k_pairs_pick_filter<Model>
//                                         the pairs calls: everything but the draws, over the pair records (PairJobHost)
//   k_seeded_round<Model, NW>, k_seeded_update
//                                         the seeded pairs call: rounds of trials that draw their own samples, and the per-pair
//                                         best, stopping rule and trial count after each round
#include "akz_fmatrix_normalised.hpp"
#include "akz_homography.hpp"
#include "akz_ransac_device.hpp"
#include "akz_ransac_seeded.hpp"

namespace akz {
namespace {

using PairJob = launch::PairJobHost;

constexpr int RT = 256;

// pts: x0 | y0 | x1 | y1, n floats each; samples: 8 match indices per trial; out: per trial 9 floats (model) and the
// inlier count (-1: no model).  The first wave forms the model, its lanes 0 .. 3 the rotations; the 256 threads count.
__global__ void __launch_bounds__(RT) k_ransac_trials(const float* __restrict__ pts, unsigned n, const unsigned* __restrict__ samples,
                                                      float epsilon_model, float epsilon_inlier, float* __restrict__ models,
                                                      int* __restrict__ inliers) {
    __shared__ float s_f[9];
    __shared__ int s_ok, s_cnt;
    __shared__ double s_m[8 * 9];
    const unsigned trial = blockIdx.x, tid = threadIdx.x;
    const float *x0 = pts, *y0 = pts + n, *x1 = pts + 2 * (size_t)n, *y1 = pts + 3 * (size_t)n;
    if (tid < 64) {
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
        wave_sync();
        for (int sweep = 0; sweep < 60; ++sweep)
            if (__ballot(jacobi_sweep_levels<8>(m, (int)tid, tid < 4)) == 0ull) break;
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

// ---- the pairs calls -------------------------------------------------------------------------------------------------------
// x0 | y0 | x1 | y1 of every match of every pair (the four arrays the host path builds), at the pair's offset of the matches:
// a workgroup per pair (grid-stride over pairs), a thread per match
__global__ void __launch_bounds__(256) k_pair_points(const PairJob* __restrict__ pairs, unsigned n_pairs, const akz_match* __restrict__ raw,
                                                     const unsigned long long* __restrict__ raw_cnt, const float* __restrict__ kx,
                                                     const float* __restrict__ ky, float* __restrict__ pts, unsigned long long stride) {
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const PairJob pj = pairs[p];
        const unsigned long long n = raw_cnt[pj.cnt_idx];
        for (unsigned long long i = threadIdx.x; i < n; i += blockDim.x) {
            const akz_match m = raw[pj.raw_off + i];
            const size_t o = pj.raw_off + i, a = pj.kp0_off + m.index_0, b = pj.kp1_off + m.index_1;
            pts[o] = kx[a];
            pts[stride + o] = ky[a];
            pts[2 * stride + o] = kx[b];
            pts[3 * stride + o] = ky[b];
        }
    }
}

// The device half of a model (the host half: FundamentalRansac / HomographyRansac): how the four lanes of a trial write its
// design rows (false: the sample gives no model, the trial never sweeps), what they keep beside the matrix, and the model
// from the rotated matrix on one lane.
struct FundamentalDev : FundamentalRansac {
    static constexpr int kRows = 8;  // rows of the trial's matrix in LDS
    struct Side {};
    // rows sub and sub + 4; every sample is usable
    static __device__ bool rows(LdsMat m, Side&, int sub, const unsigned* smp, size_t off, const float* pts, unsigned long long stride) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = sub + 4 * h;
            const size_t j = off + smp[i];
            design_row(m, i, pts[j], pts[stride + j], pts[2 * stride + j], pts[3 * stride + j]);
        }
        return true;
    }
    static __device__ bool model(LdsMat m, const Side&, float epsilon, float (&f)[9]) { return model_from_rotated(m, epsilon, f); }
};
struct HomographyDev : HomographyRansac {
    static constexpr int kRows = 8;
    struct Side {
        double v[6];  // c0x, c0y, s0, c1x, c1y, s1
    };
    // each lane loads the whole sample and forms its normalisation and degeneracy test itself (the same operands in the same
    // order: the same bits on all four), then writes the two rows of its own correspondence
    static __device__ bool rows(LdsMat m, Side& side, int sub, const unsigned* smp, size_t off, const float* pts, unsigned long long stride) {
        float x0[4], y0[4], x1[4], y1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t j = off + smp[i];
            x0[i] = pts[j]; y0[i] = pts[stride + j]; x1[i] = pts[2 * stride + j]; y1[i] = pts[3 * stride + j];
        }
        HomSample hs;
        if (!hom_prepare(x0, y0, x1, y1, hs)) return false;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i == sub) hom_rows(m, i, hs.x0[i], hs.y0[i], hs.x1[i], hs.y1[i]);
        if (sub == 0) {
            side.v[0] = hs.c0x; side.v[1] = hs.c0y; side.v[2] = hs.s0;
            side.v[3] = hs.c1x; side.v[4] = hs.c1y; side.v[5] = hs.s1;
        }
        return true;
    }
    static __device__ bool model(LdsMat m, const Side& t, float epsilon, float (&h)[9]) {
        return hom_model_from_rotated(m, epsilon, t.v[0], t.v[1], t.v[2], t.v[3], t.v[4], t.v[5], h);
    }
};

// The normalised 8-point model (akz_fmatrix_normalised.hpp; the seeded kernels only): the 9 x 9 normal matrix of the refit.
// Lane j of the trial's four takes elements j and j + 4 of every sum over the sample (sum8_part) and the four parts combine
// by two exchanges inside the quad in the order of sum8_join -- IEEE addition commutes, so all four lanes hold the bits of the
// host's sum, and with them the same centroids and scales.  The 36 sums of pass 3 thus cost each lane two points, not eight,
// and stay in registers; lane 0 writes M from them.  The rank-2 step and the denormalisation run on one lane (model).
// (the exchanges: quad_join of akz_ransac_device.hpp)
struct FundamentalNormalisedDev : FundamentalNormalisedRansac {
    static constexpr int kRows = 9;
    using Side = HomographyDev::Side;
    // (the four lanes of a trial are all here or none is, and leave together: they decide on the same bits; inlined by force --
    // left to itself the compiler calls it, and a call costs the kernel the registers of the calling convention)
    static __device__ __forceinline__ bool rows(LdsMat m, Side& side, int sub, const unsigned* smp, size_t off, const float* pts, unsigned long long stride) {
        const size_t ja = off + smp[sub], jb = off + smp[sub + 4];
        const float ax0 = pts[ja], ay0 = pts[stride + ja], ax1 = pts[2 * stride + ja], ay1 = pts[3 * stride + ja];
        const float bx0 = pts[jb], by0 = pts[stride + jb], bx1 = pts[2 * stride + jb], by1 = pts[3 * stride + jb];
        double c[4];
        {
            double a[4], b[4];
            refit_terms1(ax0, ay0, ax1, ay1, a);
            refit_terms1(bx0, by0, bx1, by1, b);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = sum8_part(a[k], b[k]);
            quad_join(c);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = c[k] / 8.0;
        }
        double s0 = 0.0, s1 = 0.0;
        {
            double a[2], b[2], d[2];
            refit_terms2(ax0, ay0, ax1, ay1, c[0], c[1], c[2], c[3], a);
            refit_terms2(bx0, by0, bx1, by1, c[0], c[1], c[2], c[3], b);
            d[0] = sum8_part(a[0], b[0]);
            d[1] = sum8_part(a[1], b[1]);
            quad_join(d);
            if (!refit_scale(d[0], 8.0, s0) || !refit_scale(d[1], 8.0, s1)) return false;
        }
        double sums[kFundRefitSums3];
        {
            double b[kFundRefitSums3];
            fund_refit_terms3(ax0, ay0, ax1, ay1, c[0], c[1], s0, c[2], c[3], s1, sums);
            fund_refit_terms3(bx0, by0, bx1, by1, c[0], c[1], s0, c[2], c[3], s1, b);
#pragma unroll
            for (int k = 0; k < kFundRefitSums3; ++k) sums[k] = sum8_part(sums[k], b[k]);
            quad_join(sums);
        }
        if (sub == 0) {
            fund_refit_normal_matrix(m, sums);
            side.v[0] = c[0]; side.v[1] = c[1]; side.v[2] = s0;
            side.v[3] = c[2]; side.v[4] = c[3]; side.v[5] = s1;
        }
        return true;
    }
    static __device__ bool model(LdsMat m, const Side& t, float epsilon, float (&f)[9]) {
        return fund_refit_model_from_rotated(m, 8.0, epsilon, t.v[0], t.v[1], t.v[2], t.v[3], t.v[4], t.v[5], f);
    }
};

// Trials first_trial .. + n_trials of a pairs call.  TPW trials per wave, four lanes per trial: a batch has ~10^5 trials, and a
// workgroup per trial with four busy lanes held a few thousand of them on the chip.  The sweeps run on each trial's four
// lanes, each trial leaving at its own first sweep without a rotation (its four ballot bits); the model is formed on one lane
// per trial; the wave then counts the inliers of its trials one after the other with all 64 lanes.  Output per trial: the
// model (9 floats) and the inlier count, or -1 (no model).
// NW > 1: the workgroup has NW - 1 more waves that only help count (a launch of few trials -- one pair, 1 000 trials, is 63
// waves -- leaves most of the chip idle while each wave counts 16 trials over every match: single homography calls on 4K pairs
// took 1.8x the fundamental-matrix call's time with one wave).  Counts are integers: the same for every NW.
constexpr int TPW = 16;  // trials per wave
constexpr int TW = 64;
template <class Model, int NW>
__global__ void __launch_bounds__(TW * NW) k_pairs_trials(const PairJob* __restrict__ pairs, const unsigned* __restrict__ trials,
                                                          unsigned long long first_trial, unsigned n_trials,
                                                          const unsigned long long* __restrict__ raw_cnt, const float* __restrict__ pts,
                                                          unsigned long long stride, float epsilon_model, float epsilon_inlier,
                                                          float* __restrict__ models, int* __restrict__ inliers) {
    constexpr int K = Model::K;
    __shared__ double s_m[TPW][8 * 9];
    __shared__ typename Model::Side s_side[TPW];
    __shared__ float s_f[TPW][9];
    __shared__ int s_ok[TPW];
    __shared__ int s_cnt[TPW];
    const int tid = (int)threadIdx.x, lane = tid & (TW - 1), tw = lane >> 2, sub = lane & 3;
    const unsigned t0 = blockIdx.x * TPW, tl = t0 + (unsigned)tw;
    if (NW == 1 || tid < TW) {  // the models: the first wave
        const bool valid = tl < n_trials;
        LdsMat m{s_m[tw]};
        bool usable = false;
        if (valid) usable = Model::rows(m, s_side[tw], sub, trials + (size_t)tl * K, pairs[trials[(size_t)n_trials * K + tl]].raw_off, pts, stride);
        wave_sync();
        bool active = usable;
        for (int sweep = 0; sweep < 60; ++sweep) {
            if (__ballot(active) == 0ull) break;
            const bool rotated = jacobi_sweep_levels<8>(m, sub, active);
            if (((__ballot(rotated) >> (4 * tw)) & 0xfull) == 0ull) active = false;  // this trial's first sweep without a rotation
        }
        if (valid && sub == 0) {
            float f[9];
            const bool ok = usable && Model::model(m, s_side[tw], epsilon_model, f);
            const size_t t = first_trial + tl;
            s_ok[tw] = ok ? 1 : 0;
            if (NW > 1) s_cnt[tw] = 0;
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
    }
    if (NW == 1) wave_sync();
    else __syncthreads();
    for (int u = 0; u < TPW; ++u) {
        const unsigned t = t0 + (unsigned)u;
        if (t >= n_trials) break;
        if (!s_ok[u]) continue;
        const PairJob pj = pairs[trials[(size_t)n_trials * K + t]];
        const unsigned n = (unsigned)raw_cnt[pj.cnt_idx];
        const float *x0 = pts + pj.raw_off, *y0 = x0 + stride, *x1 = y0 + stride, *y1 = x1 + stride;
        float f[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = s_f[u][k];
        int cnt = 0;
        for (unsigned i = (unsigned)tid; i < n; i += TW * NW) cnt += Model::inlier(f, x0[i], y0[i], x1[i], y1[i], epsilon_inlier) ? 1 : 0;
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

// ---- the seeded pairs call (akz_match_features_seeded_pairs; the statement: akz_ransac_seeded.hpp) ---------------------------------
// One round of AKZ_RANSAC_ROUND trials of every pair that still runs: workgroup 8 p + w has trials 128 round + 16 w .. + 16 of
// pair p, in the layout of k_pairs_trials (four lanes per trial, the wave counts with all lanes, NW - 1 helper waves that
// only count).  A workgroup whose pair is done, or whose trials lie at or past max_trials, leaves at once.  Each trial forms its
// own sample from (seed key k1, stream stream_base + p, trial) on its first lane -- no sample buffer, no host draw -- and hands
// it to its four lanes through LDS.  Models and counts go to slot (trial mod 128) of the pair's ring; no model: the count -1.
constexpr unsigned WPR = AKZ_RANSAC_ROUND / TPW;  // workgroups per pair and round
template <class Model, int NW>
__global__ void __launch_bounds__(TW * NW) k_seeded_round(const PairJob* __restrict__ pairs, const unsigned* __restrict__ done,
                                                          unsigned long long k1, unsigned long long stream_base, unsigned round,
                                                          unsigned max_trials, const unsigned long long* __restrict__ raw_cnt,
                                                          const float* __restrict__ pts, unsigned long long stride, float epsilon_model,
                                                          float epsilon_inlier, float* __restrict__ ring_mdl, int* __restrict__ ring_inl) {
    constexpr int K = Model::K, ROWS = Model::kRows;
    __shared__ double s_m[TPW][ROWS * 9];
    __shared__ typename Model::Side s_side[TPW];
    __shared__ float s_f[TPW][9];
    __shared__ unsigned s_smp[TPW][8];
    __shared__ int s_ok[TPW];
    __shared__ int s_cnt[TPW];
    const int tid = (int)threadIdx.x, lane = tid & (TW - 1), tw = lane >> 2, sub = lane & 3;
    const unsigned p = blockIdx.x / WPR, slot0 = (blockIdx.x % WPR) * TPW, t0 = round * AKZ_RANSAC_ROUND + slot0;
    if (done[p] != 0u || t0 >= max_trials) return;  // (the same for the whole workgroup)
    const unsigned here = min((unsigned)TPW, max_trials - t0);  // trials of this workgroup
    const PairJob pj = pairs[p];
    const unsigned n = (unsigned)raw_cnt[pj.cnt_idx];
    float* mdl = ring_mdl + (size_t)p * AKZ_RANSAC_ROUND * 9;
    int* inl = ring_inl + (size_t)p * AKZ_RANSAC_ROUND;
    const unsigned long long ks = seeded_stream_key(k1, stream_base + p);  // (uniform: the pair's stream)
    if (NW == 1 || tid < TW) {  // the models: the first wave
        const bool valid = (unsigned)tw < here;
        LdsMat m{s_m[tw]};
        if (valid && sub == 0) {
            unsigned smp[K];
            seeded_sample<K>(ks, (unsigned long long)t0 + (unsigned)tw, n, smp);
#pragma unroll
            for (int i = 0; i < K; ++i) s_smp[tw][i] = smp[i];
        }
        wave_sync();
        bool usable = false;
        if (valid) usable = Model::rows(m, s_side[tw], sub, s_smp[tw], pj.raw_off, pts, stride);
        wave_sync();
        bool active = usable;
        for (int sweep = 0; sweep < 60; ++sweep) {
            if (__ballot(active) == 0ull) break;
            const bool rotated = jacobi_sweep_levels<ROWS>(m, sub, active);
            if (((__ballot(rotated) >> (4 * tw)) & 0xfull) == 0ull) active = false;  // this trial's first sweep without a rotation
        }
        if (valid && sub == 0) {
            float f[9];
            const bool ok = usable && Model::model(m, s_side[tw], epsilon_model, f);
            const unsigned slot = slot0 + (unsigned)tw;
            s_ok[tw] = ok ? 1 : 0;
            if (NW > 1) s_cnt[tw] = 0;
            if (ok) {
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    s_f[tw][k] = f[k];
                    mdl[slot * 9 + k] = f[k];
                }
            } else {
                inl[slot] = -1;
            }
        }
    }
    if (NW == 1) wave_sync();
    else __syncthreads();
    const float *x0 = pts + pj.raw_off, *y0 = x0 + stride, *x1 = y0 + stride, *y1 = x1 + stride;
    for (unsigned u = 0; u < here; ++u) {
        if (!s_ok[u]) continue;
        float f[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = s_f[u][k];
        int cnt = 0;
        for (unsigned i = (unsigned)tid; i < n; i += TW * NW) cnt += Model::inlier(f, x0[i], y0[i], x1[i], y1[i], epsilon_inlier) ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (NW == 1) {
            if (lane == 0) inl[slot0 + u] = cnt;
        } else if (lane == 0) {
            atomicAdd(&s_cnt[u], cnt);
        }
    }
    if (NW > 1) {
        __syncthreads();
        if ((unsigned)tid < here && s_ok[tid]) inl[slot0 + (unsigned)tid] = s_cnt[tid];
    }
}

// After a round, one wave per pair that still runs: the round's first maximum (the largest count, the lowest trial among
// equals) replaces the pair's running best only if it is strictly greater -- a later tie never does -- and its model goes to the
// pair's best slot; trials_run = the trials done so far, T; the pair is done if best >= need[need_index] (need: the host's table
// of seeded_need for the rounds of one window, need_stride entries per pair; null: no stopping rule) or T == max_trials; else it
// counts in running[round].
template <int MF>  // floats of a model: 9, the resection's 15
__global__ void __launch_bounds__(TW) k_seeded_update(unsigned round, unsigned max_trials, const unsigned* __restrict__ need,
                                                      unsigned need_stride, unsigned need_index,
                                                      const float* __restrict__ ring_mdl, const int* __restrict__ ring_inl,
                                                      unsigned* __restrict__ done, int* __restrict__ best_inl, float* __restrict__ best_mdl,
                                                      unsigned* __restrict__ trials_run, unsigned* __restrict__ running) {
    const unsigned p = blockIdx.x, lane = threadIdx.x;
    if (done[p] != 0u) return;
    const unsigned t0 = round * AKZ_RANSAC_ROUND, cnt = min(AKZ_RANSAC_ROUND, max_trials - t0);  // (a running pair has t0 < max_trials)
    const int* inl = ring_inl + (size_t)p * AKZ_RANSAC_ROUND;
    int best = 0;
    unsigned bidx = ~0u;
    for (unsigned i = lane; i < cnt; i += TW) {
        const int v = inl[i];
        if (v > best) {
            best = v;
            bidx = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_xor(best, o, 64);
        const unsigned oi = __shfl_xor(bidx, o, 64);
        if (ob > best || (ob == best && oi < bidx)) {
            best = ob;
            bidx = oi;
        }
    }
    const int before = best_inl[p];
    if (best > before && lane < MF) best_mdl[(size_t)p * MF + lane] = ring_mdl[((size_t)p * AKZ_RANSAC_ROUND + bidx) * MF + lane];
    if (lane == 0) {
        const unsigned T = t0 + cnt, now = (unsigned)max(best, before);
        if (best > before) best_inl[p] = best;
        trials_run[p] = T;
        if (T == max_trials || (need && now >= need[(size_t)p * need_stride + need_index])) done[p] = 1u;
        else atomicAdd(running + round, 1u);
    }
}

// Per pair (a workgroup, grid-stride): the winner among its trials (pick_winner; fewer than K matches: none), and the matches
// it keeps (Model::inlier, as the host's final filter), compacted in match order.  Fewer than K matches: all kept.  No winner:
// the zero model is evaluated, or (kKeepAllWithoutWinner) all kept.  h_out / found_out, where the call hands the model back (else
// null): the winner's model or zeros, and found.
template <class Model>
__global__ void __launch_bounds__(kGroup) k_pairs_pick_filter(const PairJob* __restrict__ pairs, unsigned n_pairs, const akz_match* __restrict__ raw,
                                                              const unsigned long long* __restrict__ raw_cnt, const float* __restrict__ pts,
                                                              unsigned long long stride, const float* __restrict__ models,
                                                              const int* __restrict__ inliers, float epsilon_inlier, akz_match* __restrict__ keep,
                                                              unsigned long long* __restrict__ keep_cnt, float* __restrict__ h_out,
                                                              int* __restrict__ found_out) {
    __shared__ int s_best[kGroup / 64];
    __shared__ unsigned long long s_idx[kGroup / 64];
    __shared__ unsigned s_wsum[kGroup / 64];
    __shared__ float s_f[9];
    __shared__ int s_found;
    const unsigned tid = threadIdx.x;
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const PairJob pj = pairs[p];
        const unsigned long long n = raw_cnt[pj.cnt_idx];
        const Winner win = pick_winner(inliers, pj.trial_off, pj.n_trials, n >= (unsigned long long)Model::K, s_best, s_idx, tid);
        if (tid == 0) {
            const int found = win.best > 0 ? 1 : 0;
            if (Model::kKeepAllWithoutWinner) s_found = found;
            for (int k = 0; k < 9; ++k) {
                s_f[k] = found ? models[(pj.trial_off + win.bidx) * 9 + k] : 0.0f;
                if (h_out) h_out[(size_t)p * 9 + k] = s_f[k];
            }
            if (found_out) found_out[p] = found;
        }
        __syncthreads();
        const bool all = n < (unsigned long long)Model::K || (Model::kKeepAllWithoutWinner && s_found == 0);
        float f[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = s_f[k];
        const float *x0 = pts + pj.raw_off, *y0 = x0 + stride, *x1 = y0 + stride, *y1 = x1 + stride;
        unsigned long long written = 0;
        for (unsigned long long base = 0; base < n; base += kGroup) {
            const unsigned long long i = base + tid;
            const bool kept = i < n && (all || Model::inlier(f, x0[i], y0[i], x1[i], y1[i], epsilon_inlier));
            compact_kept(kept, raw + pj.raw_off + i, keep + pj.keep_off, written, s_wsum, tid);
        }
        if (tid == 0) keep_cnt[p] = written;
    }
}

}  // namespace

namespace launch {
void pair_points(hipStream_t s, const PairJobHost* d_pairs, uint32_t n_pairs, const void* d_raw, const uint64_t* d_raw_cnt,
                 const float* d_kx, const float* d_ky, float* d_pts, uint64_t pts_stride) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(k_pair_points, dim3(std::min<uint32_t>(n_pairs, 8192)), dim3(256), 0, s, d_pairs, n_pairs, (const akz_match*)d_raw,
                       (const unsigned long long*)d_raw_cnt, d_kx, d_ky, d_pts, (unsigned long long)pts_stride);
}
void pairs_trials(hipStream_t s, RansacModel model, const PairJobHost* d_pairs, const uint32_t* d_trials, uint64_t first_trial,
                  uint32_t n_trials, const uint64_t* d_raw_cnt, const float* d_pts, uint64_t pts_stride, float epsilon_model,
                  float epsilon_inlier, float* d_models, int32_t* d_inliers) {
    if (n_trials == 0) return;
    // the fundamental matrix: one wave per workgroup, the waves share nothing.  The homography with fewer workgroups than half
    // the chip's SIMDs (256 CUs x 4): three helper waves per workgroup for the counts
    const uint32_t blocks = (n_trials + TPW - 1) / TPW;
    auto k = model == RansacModel::Fundamental ? k_pairs_trials<FundamentalDev, 1>
             : blocks < 512                    ? k_pairs_trials<HomographyDev, 4>
                                               : k_pairs_trials<HomographyDev, 1>;
    const uint32_t nw = model == RansacModel::Homography && blocks < 512 ? 4 : 1;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(TW * nw), 0, s, d_pairs, d_trials, (unsigned long long)first_trial, n_trials,
                       (const unsigned long long*)d_raw_cnt, d_pts, (unsigned long long)pts_stride, epsilon_model, epsilon_inlier, d_models,
                       d_inliers);
}
void seeded_round(hipStream_t s, RansacModel model, const PairJobHost* d_pairs, uint32_t n_pairs, const uint32_t* d_done, uint64_t k1,
                  uint64_t stream_base, uint32_t round, uint32_t max_trials, const uint64_t* d_raw_cnt, const float* d_pts, uint64_t pts_stride,
                  float epsilon_model, float epsilon_inlier, float* d_ring_mdl, int32_t* d_ring_inl) {
    if (n_pairs == 0) return;
    // Helper waves, as k_pairs_trials has them for small launches, here for both models: a round is 8 workgroups per pair by
    // construction, so below 64 pairs (512 workgroups: half the chip's SIMDs) a lone wave per workgroup would count its 16
    // trials over every match with most of the chip idle.  Counts are integers: the same for every NW.
    const uint32_t blocks = n_pairs * WPR;
    const bool helpers = blocks < 512;
    auto k = model == RansacModel::Fundamental ? (helpers ? k_seeded_round<FundamentalDev, 4> : k_seeded_round<FundamentalDev, 1>)
             : model == RansacModel::Homography
                 ? (helpers ? k_seeded_round<HomographyDev, 4> : k_seeded_round<HomographyDev, 1>)
                 : (helpers ? k_seeded_round<FundamentalNormalisedDev, 4> : k_seeded_round<FundamentalNormalisedDev, 1>);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(TW * (helpers ? 4 : 1)), 0, s, d_pairs, d_done, (unsigned long long)k1,
                       (unsigned long long)stream_base, round, max_trials, (const unsigned long long*)d_raw_cnt, d_pts,
                       (unsigned long long)pts_stride, epsilon_model, epsilon_inlier, d_ring_mdl, d_ring_inl);
}
void seeded_update(hipStream_t s, uint32_t n_pairs, uint32_t round, uint32_t max_trials, const uint32_t* d_need, uint32_t need_stride,
                   uint32_t need_index, const float* d_ring_mdl, const int32_t* d_ring_inl, uint32_t* d_done, int32_t* d_best_inl, float* d_best_mdl,
                   uint32_t* d_trials_run, uint32_t* d_running, uint32_t model_floats) {
    if (n_pairs == 0) return;
    auto k = model_floats == 9 ? k_seeded_update<9> : k_seeded_update<15>;
    hipLaunchKernelGGL(k, dim3(n_pairs), dim3(TW), 0, s, round, max_trials, d_need, need_stride, need_index, d_ring_mdl, d_ring_inl, d_done,
                       d_best_inl, d_best_mdl, d_trials_run, d_running);
}
void pairs_pick_filter(hipStream_t s, RansacModel model, const PairJobHost* d_pairs, uint32_t n_pairs, const void* d_raw,
                       const uint64_t* d_raw_cnt, const float* d_pts, uint64_t pts_stride, const float* d_models, const int32_t* d_inliers,
                       float epsilon_inlier, void* d_keep, uint64_t* d_keep_cnt, float* d_h, int32_t* d_found) {
    if (n_pairs == 0) return;
    auto k = model == RansacModel::Fundamental  ? k_pairs_pick_filter<FundamentalDev>
             : model == RansacModel::Homography ? k_pairs_pick_filter<HomographyDev>
                                                : k_pairs_pick_filter<FundamentalNormalisedDev>;
    hipLaunchKernelGGL(k, dim3(std::min<uint32_t>(n_pairs, 8192)), dim3(kGroup), 0, s, d_pairs, n_pairs, (const akz_match*)d_raw,
                       (const unsigned long long*)d_raw_cnt, d_pts, (unsigned long long)pts_stride, d_models, d_inliers, epsilon_inlier,
                       (akz_match*)d_keep, (unsigned long long*)d_keep_cnt, d_h, d_found);
}
void ransac_trials(hipStream_t s, const float* d_pts, uint32_t n_matches, const uint32_t* d_samples, uint32_t trials, float epsilon_model,
                   float epsilon_inlier, float* d_models, int32_t* d_inliers) {
    if (trials == 0) return;
    hipLaunchKernelGGL(k_ransac_trials, dim3(trials), dim3(RT), 0, s, d_pts, n_matches, d_samples, epsilon_model, epsilon_inlier, d_models,
                       d_inliers);
}
}  // namespace launch
}  // namespace akz
