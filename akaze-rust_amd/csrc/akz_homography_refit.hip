// The refit stage of akz_match_features_homography_refined(_pairs) and akz_match_features_fundamental_refined(_pairs): after
// k_pairs_pick_filter (akz_ransac_kernels.hip) has left every pair's winner, found flag and kept list on the device, this
// kernel runs the local optimisation of akz_homography_refit.hpp on the pair's RAW list -- the same source as the host
// statements akz_refine_homography and akz_refine_fundamental_matrix, the same bits -- and rewrites the model, the kept list
// and its count.  One loop for every model (refit_loop of akz_ransac_device.hpp): k_refit<R> with R = HomographyRefit (akz_homography_refit.hpp), FundamentalRefit
// (akz_fundamental_refit.hpp) or, for the seeded call's third kind, FundamentalNormalisedRefit (akz_fmatrix_normalised.hpp:
// FundamentalRefit with the Sampson rule).
#include "akz_fmatrix_normalised.hpp"
#include "akz_fundamental_refit.hpp"
#include "akz_homography_refit.hpp"
#include "akz_ransac_device.hpp"

namespace akz {
namespace {

// Per pair (a workgroup of 256, grid-stride): nothing for a pair without a model, with fewer than R::kMin matches (4: H, 8: F)
// or with max_iterations == 0 (iterations = 0, the model and the kept list stay the pick kernel's); else refit_loop over the
// pair's raw list (24 lane sums in pass 3 for H, 36 for F; F's model tail with the rank-2 step, its three rows in the LDS of M).
// After at least one accepted fit: the model rewritten, the kept list compacted again in match order, keep_cnt rewritten.
// (two waves a SIMD, stated: the fundamental matrix's instances need every one of the 256 registers that leaves them, and left to
// itself the allocator takes a few more and halves the occupancy)
template <class R>
__global__ void __launch_bounds__(kGroup, 2) k_refit(PairTable table, unsigned n_pairs, const akz_match* __restrict__ raw, float epsilon_model,
                                              float epsilon_inlier, unsigned max_iterations, akz_match* __restrict__ keep,
                                              unsigned long long* __restrict__ keep_cnt, float* __restrict__ h_io,
                                              const int* __restrict__ found, unsigned* __restrict__ iterations) {
    __shared__ unsigned s_wsum[kGroup / 64];
    const unsigned tid = threadIdx.x;
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const launch::PairJobHost pj = table.pairs[p];
        const unsigned long long n64 = table.raw_cnt[pj.cnt_idx];
        if (found[p] == 0 || n64 < (unsigned long long)R::kMin || max_iterations == 0) {  // (the same for the whole workgroup)
            if (tid == 0) iterations[p] = 0;
            continue;
        }
        const PairView v = table.view(p);
        float h[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) h[k] = h_io[(size_t)p * 9 + k];
        const unsigned done = refit_loop<R>(v, h, epsilon_model, epsilon_inlier, max_iterations, s_wsum, tid);
        if (done > 0) {
            if (tid == 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) h_io[(size_t)p * 9 + k] = h[k];
            }
            unsigned long long written = 0;
            for (unsigned base = 0; base < v.n; base += kGroup) {
                const unsigned i = base + tid;
                const bool kept = i < v.n && R::inlier(h, v, i, epsilon_inlier);
                compact_kept(kept, raw + pj.raw_off + i, keep + pj.keep_off, written, s_wsum, tid);
            }
            if (tid == 0) keep_cnt[p] = written;
        }
        if (tid == 0) iterations[p] = done;
        __syncthreads();  // (refit_loop's LDS: the next pair's)
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
    hipLaunchKernelGGL(k, dim3(std::min<uint32_t>(n_pairs, 8192)), dim3(kGroup), 0, s,
                       PairTable{d_pairs, (const unsigned long long*)d_raw_cnt, d_pts, pts_stride}, n_pairs, (const akz_match*)d_raw, epsilon_model,
                       epsilon_inlier, max_iterations, (akz_match*)d_keep, (unsigned long long*)d_keep_cnt, d_h, d_found, d_iterations);
}
}  // namespace launch
}  // namespace akz
