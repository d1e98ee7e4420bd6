// The refit stage of akz_match_features_homography_refined(_pairs) and akz_match_features_fundamental_refined(_pairs): after
// k_pairs_pick_filter (akz_ransac_kernels.hip) has left every pair's winner, found flag and kept list on the device, this
// kernel runs the local optimisation of akz_homography_refit.hpp on the pair's RAW list -- the same source as the host
// statements akz_refine_homography and akz_refine_fundamental_matrix, the same bits -- and rewrites the model, the kept list
// and its count.  One loop for every model: k_refit<R> with R = HomographyRefit (akz_homography_refit.hpp), FundamentalRefit
// (akz_fundamental_refit.hpp) or, for the seeded call's third kind, FundamentalNormalisedRefit (akz_fmatrix_normalised.hpp:
// FundamentalRefit with the Sampson rule).
#include "akz_fmatrix_normalised.hpp"
#include "akz_fundamental_refit.hpp"
#include "akz_homography_refit.hpp"
#include "akz_ransac_device.hpp"

namespace akz {
namespace {

using PairJob = launch::PairJobHost;

constexpr int RF = kRefitLanes;  // one thread per lane of the summation order
static_assert(RF == kGroup, "compact_kept");
constexpr int RG = kSumGroup;    // sums that go through the tree together (block_sums; LDS: RG x 256 doubles)

// |{ i < n : inlier under h }| for every thread
template <class R>
__device__ unsigned block_count(const float (&h)[9], const float* x0, const float* y0, const float* x1, const float* y1, unsigned n,
                                float eps, unsigned* s_wsum, unsigned tid) {
    unsigned cnt = 0;
    for (unsigned i = tid; i < n; i += RF) cnt += R::inlier(h, x0[i], y0[i], x1[i], y1[i], eps) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63u) == 0) s_wsum[tid >> 6] = cnt;
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int k = 0; k < RF / 64; ++k) total += s_wsum[k];
    __syncthreads();
    return total;
}

// Per pair (a workgroup of 256, grid-stride): nothing for a pair without a model, with fewer than R::kMin matches (4: H, 8: F)
// or with max_iterations == 0 (iterations = 0, the model and the kept list stay the pick kernel's); else the loop of the
// statement.  Element i of the raw list is thread i mod 256's, added in ascending i: the lane sums live in f64 registers (24
// in pass 3 for H, 36 for F; they go through the tree six at a time).  The 9 x 9 decomposition keeps M in LDS, as the trial
// kernel keeps its 8 x 9: its rotations run on four lanes (jacobi_sweep_levels<9>: 15 levels per sweep); the smallest row, the
// rank rule and the model tail (F: with the rank-2 step, its three rows in the LDS of M) on thread 0.  After at least one
// accepted fit: the model rewritten, the kept list compacted again in match order, keep_cnt rewritten.
template <class R>
__global__ void __launch_bounds__(RF) k_refit(const PairJob* __restrict__ pairs, unsigned n_pairs, const akz_match* __restrict__ raw,
                                                         const unsigned long long* __restrict__ raw_cnt, const float* __restrict__ pts,
                                                         unsigned long long stride, float epsilon_model, float epsilon_inlier,
                                                         unsigned max_iterations, akz_match* __restrict__ keep,
                                                         unsigned long long* __restrict__ keep_cnt, float* __restrict__ h_io,
                                                         const int* __restrict__ found, unsigned* __restrict__ iterations) {
    __shared__ double s_red[RG * RF];
    __shared__ double s_sum[R::kSums3];
    __shared__ double s_m[9 * 9];
    __shared__ float s_h[9];
    __shared__ int s_ok;
    __shared__ unsigned s_wsum[RF / 64];
    const unsigned tid = threadIdx.x;
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const PairJob pj = pairs[p];
        const unsigned long long n64 = raw_cnt[pj.cnt_idx];
        if (found[p] == 0 || n64 < (unsigned long long)R::kMin || max_iterations == 0) {  // (the same for the whole workgroup)
            if (tid == 0) iterations[p] = 0;
            continue;
        }
        const unsigned n = (unsigned)n64;
        const float *x0 = pts + pj.raw_off, *y0 = x0 + stride, *x1 = y0 + stride, *y1 = x1 + stride;
        float h[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) h[k] = h_io[(size_t)p * 9 + k];
        unsigned cnt = block_count<R>(h, x0, y0, x1, y1, n, epsilon_inlier, s_wsum, tid);
        unsigned done = 0;
        while (done < max_iterations) {
            if (cnt < (unsigned)R::kMin) break;
            const double count = (double)cnt;
            double c0x, c0y, c1x, c1y, s0 = 0.0, s1 = 0.0;
            {
                double v[4] = {0.0, 0.0, 0.0, 0.0};
                for (unsigned i = tid; i < n; i += RF)
                    if (R::inlier(h, x0[i], y0[i], x1[i], y1[i], epsilon_inlier)) {
                        double t[4];
                        refit_terms1(x0[i], y0[i], x1[i], y1[i], t);
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = v[k] + t[k];
                    }
                block_sums<4>(v, s_red, s_sum, tid);
                c0x = s_sum[0] / count; c0y = s_sum[1] / count; c1x = s_sum[2] / count; c1y = s_sum[3] / count;
            }
            {
                double v[2] = {0.0, 0.0};
                for (unsigned i = tid; i < n; i += RF)
                    if (R::inlier(h, x0[i], y0[i], x1[i], y1[i], epsilon_inlier)) {
                        double t[2];
                        refit_terms2(x0[i], y0[i], x1[i], y1[i], c0x, c0y, c1x, c1y, t);
                        v[0] = v[0] + t[0];
                        v[1] = v[1] + t[1];
                    }
                block_sums<2>(v, s_red, s_sum, tid);
                const double d0 = s_sum[0], d1 = s_sum[1];
                if (!refit_scale(d0, count, s0) || !refit_scale(d1, count, s1)) break;  // (the same for every thread)
            }
            {
                double v[R::kSums3];
#pragma unroll
                for (int k = 0; k < R::kSums3; ++k) v[k] = 0.0;
                for (unsigned i = tid; i < n; i += RF)
                    if (R::inlier(h, x0[i], y0[i], x1[i], y1[i], epsilon_inlier)) {
                        double t[R::kSums3];
                        R::terms3(x0[i], y0[i], x1[i], y1[i], c0x, c0y, s0, c1x, c1y, s1, t);
#pragma unroll
                        for (int k = 0; k < R::kSums3; ++k) v[k] = v[k] + t[k];
                    }
                block_sums<R::kSums3>(v, s_red, s_sum, tid);
            }
            if (tid < 64) {  // the first wave: M, the sweeps on its lanes 0 .. 3, the model on lane 0
                LdsMat m{s_m};
                if (tid == 0) R::normal_matrix(m, s_sum);
                wave_sync();
                for (int sweep = 0; sweep < 60; ++sweep)
                    if (__ballot(jacobi_sweep_levels<9>(m, (int)tid, tid < 4)) == 0ull) break;  // the first sweep without a rotation
                if (tid == 0) {
                    float h2[9];
                    const bool ok = R::model_from_rotated(m, count, epsilon_model, c0x, c0y, s0, c1x, c1y, s1, h2);
                    s_ok = ok ? 1 : 0;
                    if (ok) {
#pragma unroll
                        for (int k = 0; k < 9; ++k) s_h[k] = h2[k];
                    }
                }
            }
            __syncthreads();
            if (s_ok == 0) break;
            float h2[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) h2[k] = s_h[k];
            const unsigned cnt2 = block_count<R>(h2, x0, y0, x1, y1, n, epsilon_inlier, s_wsum, tid);
            if (cnt2 < cnt) break;  // h2 is rejected
            const bool grew = cnt2 > cnt;
#pragma unroll
            for (int k = 0; k < 9; ++k) h[k] = h2[k];
            cnt = cnt2;
            ++done;
            if (!grew) break;
        }
        if (done > 0) {
            if (tid == 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) h_io[(size_t)p * 9 + k] = h[k];
            }
            unsigned long long written = 0;
            for (unsigned base = 0; base < n; base += RF) {
                const unsigned i = base + tid;
                const bool kept = i < n && R::inlier(h, x0[i], y0[i], x1[i], y1[i], epsilon_inlier);
                compact_kept(kept, raw + pj.raw_off + i, keep + pj.keep_off, written, s_wsum, tid);
            }
            if (tid == 0) keep_cnt[p] = written;
        }
        if (tid == 0) iterations[p] = done;
        __syncthreads();  // (s_ok, s_h, s_sum: the next pair's)
    }
}

}  // namespace

namespace launch {
void model_refit(hipStream_t s, RansacModel model, const PairJobHost* d_pairs, uint32_t n_pairs, const void* d_raw, const uint64_t* d_raw_cnt,
                      const float* d_pts, uint64_t pts_stride, float epsilon_model, float epsilon_inlier, uint32_t max_iterations,
                      void* d_keep, uint64_t* d_keep_cnt, float* d_h, const int32_t* d_found, uint32_t* d_iterations) {
    if (n_pairs == 0) return;
    auto k = model == RansacModel::Fundamental  ? k_refit<FundamentalRefit>
             : model == RansacModel::Homography ? k_refit<HomographyRefit>
                                                : k_refit<FundamentalNormalisedRefit>;
    hipLaunchKernelGGL(k, dim3(std::min<uint32_t>(n_pairs, 8192)), dim3(RF), 0, s, d_pairs, n_pairs, (const akz_match*)d_raw,
                       (const unsigned long long*)d_raw_cnt, d_pts, (unsigned long long)pts_stride, epsilon_model, epsilon_inlier,
                       max_iterations, (akz_match*)d_keep, (unsigned long long*)d_keep_cnt, d_h, d_found, d_iterations);
}
}  // namespace launch
}  // namespace akz
