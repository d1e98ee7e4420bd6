// Local optimisation of the winning homography: the least-squares refit on its inliers and the re-classification, as ONE
// piece of source for the host statement (akz_refine_homography, akz_ransac.cpp) and the device kernel
// (k_refit<HomographyRefit>, akz_homography_refit.hip), like akz_homography.hpp for the trial model: f64 in a fixed order, no
// contraction, the same bits on both sides.
//
// The loop, over a pair's RAW match list (the set can grow):
//     S = { i : homography_inlier(h, i, eps) };  done = 0
//     while done < max_iterations:
//         h' = fit(S)            (no model: stop)
//         S' = inliers(h')
//         |S'| < |S|: stop       (h' is rejected)
//         grew = |S'| > |S|;  h, S = h', S';  done += 1
//         not grew: stop
// so the result never has fewer inliers than the input and at most min(max_iterations, n) fits are accepted.
//
// fit(S), |S| >= 4 (fewer: no model), three sums over S:
//   1. sum x0, sum y0, sum x1, sum y1 (f32 widened to f64); centroid c = sum / |S|;
//   2. per image sum |p - c| = sum sqrt(dx dx + dy dy); d = sum / |S|; d == 0 in either image: no model; s = sqrt(2) / d;
//   3. with x = s0 (x0 - c0x), y = s0 (y0 - c0y), u = s1 (x1 - c1x), v = s1 (y1 - c1y) and a = {x x, x y, x, y y, y, 1} (the
//      six distinct entries of (x, y, 1)(x, y, 1)^T): sum a[k], sum u a[k], sum v a[k], sum (u u + v v) a[k] -- 24 sums.
//      They are the blocks P, Q_u, Q_v, R of the normal matrix M = A^T A of the rows hom_rows writes:
//          M = [[P, 0, -Q_u], [0, P, -Q_v], [-Q_u, -Q_v, R]]   (9 x 9, symmetric).
// EVERY sum is formed in one order: element i (its position in the raw list) belongs to lane i mod 256; a lane adds its
// members in ascending i starting from +0.0; the 256 lane sums combine by p[l] = p[l] + p[l + s] for s = 128, 64, .., 1
// (l < s); p[0] is the sum.  (The host keeps a 256-entry array, the device a register per thread, LDS for s = 128, 64 and
// __shfl_down for s = 32 .. 1, whose lane 0 receives exactly that order.)
//
// Null vector of M: the one-sided Jacobi sweeps of akz_fmatrix.hpp on the 9 rows of M (jacobi_sweeps_rows<9>).  The rotated
// rows are orthogonal, row i is lambda_i v_i^T (M symmetric: eigenvalue times eigenvector), its norm lambda_i = sigma_i(A)^2.
// The row of the smallest norm (the first among equals) is dropped: row 8 is copied over it, so rows 0..7 are the kept ones.
// Rank rule: every kept norm must exceed epsilon_model^2 |S| / 4 -- M's units are those of A squared and its entries are sums
// over S, so for |S| = 4 this is the trial model's sigma_i(A) > epsilon_model -- else no model.  The kept rows go to
// hom_model_from_rows (the projection tail of the trial model, robust when lambda_9 ~ 0, as it is for exact data), which also
// denormalises, applies the H[8] rule and rounds to f32.
// Forming A^T A squares the condition number (see the note in akz_fmatrix.hpp).  On Hartley-normalised points the design
// matrix has a condition of 1e1 .. 1e3 over its eight non-zero singular values, so the squared 1e6 leaves ten digits in f64:
// harmless here, unlike the raw pixel coordinates that note speaks of.
#pragma once
#include <cstddef>
#include <cstdint>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <cstring>
#include <vector>
#endif

#include "akz_homography.hpp"

namespace akz {

constexpr int kRefitLanes = 256;  // lanes of the summation order
constexpr int kRefitSums3 = 24;   // sums of pass 3

AKZ_HD void refit_terms1(float x0, float y0, float x1, float y1, double (&t)[4]) {
    t[0] = (double)x0;
    t[1] = (double)y0;
    t[2] = (double)x1;
    t[3] = (double)y1;
}
AKZ_HD void refit_terms2(float x0, float y0, float x1, float y1, double c0x, double c0y, double c1x, double c1y, double (&t)[2]) {
    const double dx0 = (double)x0 - c0x, dy0 = (double)y0 - c0y, dx1 = (double)x1 - c1x, dy1 = (double)y1 - c1y;
    t[0] = sqrt(dx0 * dx0 + dy0 * dy0);
    t[1] = sqrt(dx1 * dx1 + dy1 * dy1);
}
// t[k] = a[k], t[6 + k] = u a[k], t[12 + k] = v a[k], t[18 + k] = (u u + v v) a[k]
AKZ_HD void refit_terms3(float x0, float y0, float x1, float y1, double c0x, double c0y, double s0, double c1x, double c1y, double s1,
                         double (&t)[kRefitSums3]) {
    const double x = s0 * ((double)x0 - c0x), y = s0 * ((double)y0 - c0y);
    const double u = s1 * ((double)x1 - c1x), v = s1 * ((double)y1 - c1y);
    const double a[6] = {x * x, x * y, x, y * y, y, 1.0};
    const double w = u * u + v * v;
    AKZ_UNROLL
    for (int k = 0; k < 6; ++k) {
        t[k] = a[k];
        t[6 + k] = u * a[k];
        t[12 + k] = v * a[k];
        t[18 + k] = w * a[k];
    }
}
// centroid and scale of one image from its sums; false: d == 0
AKZ_HD bool refit_scale(double sum_d, double count, double& s) {
    const double d = sum_d / count;
    if (!(d > 0.0)) return false;
    s = 1.4142135623730951 / d;  // sqrt(2) / d
    return true;
}

// M (9 x 9: m.at(r, k), r, k < 9) from the 24 sums of pass 3
template <class M>
AKZ_HD void refit_normal_matrix(M& m, const double* sums) {
    AKZ_UNROLL
    for (int i = 0; i < 3; ++i) {
        AKZ_UNROLL
        for (int j = 0; j < 3; ++j) {
            // index of (i, j) among the six distinct entries of the symmetric 3 x 3
            const int k = i <= j ? (i == 0 ? j : (i == 1 ? 2 + j : 5)) : (j == 0 ? i : (j == 1 ? 2 + i : 5));
            const double p = sums[k], qu = sums[6 + k], qv = sums[12 + k], r = sums[18 + k];
            m.at(i, j) = p;
            m.at(i, 3 + j) = 0.0;
            m.at(i, 6 + j) = -qu;
            m.at(3 + i, j) = 0.0;
            m.at(3 + i, 3 + j) = p;
            m.at(3 + i, 6 + j) = -qv;
            m.at(6 + i, j) = -qu;
            m.at(6 + i, 3 + j) = -qv;
            m.at(6 + i, 6 + j) = r;
        }
    }
}

// the model from the rotated M (after the sweeps) and the normalisation: the dropped row, the rank rule, the shared tail;
// count = |S|
template <class M>
AKZ_HD bool refit_model_from_rotated(M& m, double count, float epsilon_model, double c0x, double c0y, double s0, double c1x, double c1y,
                                     double s1, float (&h)[9]) {
    int mi = 0;
    double smallest = 0.0;
    AKZ_NOUNROLL
    for (int i = 0; i < 9; ++i) {
        double nrm = 0.0;
        AKZ_UNROLL
        for (int k = 0; k < 9; ++k) nrm += m.at(i, k) * m.at(i, k);
        nrm = sqrt(nrm);
        if (i == 0 || nrm < smallest) {  // the first one among equals
            smallest = nrm;
            mi = i;
        }
    }
    if (mi != 8) {
        AKZ_UNROLL
        for (int k = 0; k < 9; ++k) m.at(mi, k) = m.at(8, k);
    }
    const double threshold = ((double)epsilon_model * (double)epsilon_model) * (count * 0.25);
    bool full = true;
    AKZ_NOUNROLL
    for (int i = 0; i < 8; ++i) {
        double nrm = 0.0;
        AKZ_UNROLL
        for (int k = 0; k < 9; ++k) nrm += m.at(i, k) * m.at(i, k);
        nrm = sqrt(nrm);
        if (!(nrm > threshold)) full = false;
    }
    if (!full) return false;
    return hom_model_from_rows(m, c0x, c0y, s0, c1x, c1y, s1, h);
}
// (the sweeps before it: jacobi_sweeps_rows<9> on the host; the device runs the same rotations level by level on four lanes,
// see jacobi_sweep_levels)

struct Mat9x9 {
    double v[9][9];
    AKZ_HD double& at(int p, int k) { return v[p][k]; }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// The host's form of that order, for every refit (akz_ransac.cpp, akz_resection_api.cpp): the sums of the members' terms -- lane
// i mod 256, ascending i from +0.0, then the tree.  member: n flags (any indexable); term(i, t) writes element i's K terms.
template <int K, class Members, class Term>
inline void lane_tree_sums(uint64_t n, const Members& member, Term term, double (&out)[K]) {
    static thread_local double p[K][kRefitLanes];
    for (int k = 0; k < K; ++k)
        for (int l = 0; l < kRefitLanes; ++l) p[k][l] = 0.0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!member[(size_t)i]) continue;
        double t[K];
        term(i, t);
        for (int k = 0; k < K; ++k) p[k][i % kRefitLanes] = p[k][i % kRefitLanes] + t[k];
    }
    for (int k = 0; k < K; ++k) {
        for (int s = kRefitLanes / 2; s > 0; s >>= 1)
            for (int l = 0; l < s; ++l) p[k][l] = p[k][l] + p[k][l + s];
        out[k] = p[k][0];
    }
}

// The loop of the statement on the host for every refit model R (the concept: below) over a view v of n elements -- the one place
// where the host classifies, fits and applies the accept / grew / stop rule; the device's is refit_loop of akz_ransac_device.hpp.
// h: the model to start from, the last accepted one on return; member (n flags): the final set; -> the fits accepted.
template <class R, class View>
inline uint32_t refit_loop_host(const View& v, uint64_t n, float (&h)[R::kFloats], float epsilon_model, float epsilon_inlier,
                                uint32_t max_iterations, std::vector<uint8_t>& member) {
    auto classify = [&](const float (&m)[R::kFloats], std::vector<uint8_t>& set) {
        uint64_t c = 0;
        for (uint64_t i = 0; i < n; ++i) c += set[(size_t)i] = R::inlier(m, v, i, epsilon_inlier) ? 1 : 0;
        return c;
    };
    // fit(S) over the members, |S| = count, in the tree's order; false: no model
    auto fit = [&](const std::vector<uint8_t>& set, uint64_t count, float (&h2)[R::kFloats]) {
        if (count < (uint64_t)R::kMin) return false;
        const double cnt = (double)count;
        double sum1[R::kSums1], sum2[2], sum3[R::kSums3], c[R::kSums1];
        lane_tree_sums<R::kSums1>(n, set, [&](uint64_t i, double (&t)[R::kSums1]) { R::terms1(v, i, t); }, sum1);
        for (int k = 0; k < R::kSums1; ++k) c[k] = sum1[k] / cnt;
        lane_tree_sums<2>(n, set, [&](uint64_t i, double (&t)[2]) { R::terms2(v, i, c, t); }, sum2);
        double s0 = 0.0, s1 = 0.0;
        if (!refit_scale(sum2[0], cnt, s0) || !R::scale2(sum2[1], cnt, s1)) return false;
        lane_tree_sums<R::kSums3>(n, set, [&](uint64_t i, double (&t)[R::kSums3]) { R::terms3(v, i, c, s0, s1, t); }, sum3);
        typename R::Mat m;
        R::normal_matrix(m, sum3);
        jacobi_sweeps_rows<R::kRows, R::kRows>(m);
        return R::model_from_rotated(m, cnt, epsilon_model, c, s0, s1, h2);
    };
    std::vector<uint8_t> next((size_t)n);
    uint64_t count = classify(h, member);
    uint32_t done = 0;
    while (done < max_iterations) {
        float h2[R::kFloats];
        if (!fit(member, count, h2)) break;
        const uint64_t count2 = classify(h2, next);
        if (count2 < count) break;  // h2 is rejected
        const bool grew = count2 > count;
        std::memcpy(h, h2, sizeof(h2));
        member.swap(next);
        count = count2;
        ++done;
        if (!grew) break;
    }
    return done;
}
#endif

// A REFIT model (HomographyRefit, FundamentalRefit, ResectionRefit of akz_resection.hpp): what refit_loop_host and the device's
// refit_loop need from a model, over a view v of the elements and an index i into it:
//   kMin, kFloats           the fewest members of a fit (and elements the stage works on); the floats of a model
//   kSums1, kSums3          the sums of passes 1 and 3; pass 2 has two, the first scaled by refit_scale, the second by scale2
//   kRows, Mat              M is kRows x kRows; the host's matrix type
//   inlier(h, v, i, eps), terms1(v, i, t), terms2(v, i, c, t), terms3(v, i, c, s0, s1, t)      (c: the kSums1 centroids)
//   normal_matrix(m, sums), model_from_rotated(m, count, epsilon_model, c, s0, s1, h)
// Every model of two views (a view: x0 | y0 | x1 | y1) has the passes 1 and 2 of the statement above and a 9 x 9 M:
struct TwoViewRefit {
    static constexpr int kSums1 = 4, kRows = 9, kFloats = 9;
    using Mat = Mat9x9;
    template <class V, class I>
    static AKZ_HD void terms1(const V& v, I i, double (&t)[4]) {
        refit_terms1(v.x0[i], v.y0[i], v.x1[i], v.y1[i], t);
    }
    template <class V, class I>
    static AKZ_HD void terms2(const V& v, I i, const double (&c)[4], double (&t)[2]) {
        refit_terms2(v.x0[i], v.y0[i], v.x1[i], v.y1[i], c[0], c[1], c[2], c[3], t);
    }
    static AKZ_HD bool scale2(double sum_d, double count, double& s) { return refit_scale(sum_d, count, s); }
};
// the homography (FundamentalRefit of akz_fundamental_refit.hpp is the other one of two views)
struct HomographyRefit : TwoViewRefit {
    static constexpr int kMin = 4;
    static constexpr int kSums3 = kRefitSums3;
    template <class V, class I>
    static AKZ_HD bool inlier(const float (&h)[9], const V& v, I i, float eps) {
        return homography_inlier(h, v.x0[i], v.y0[i], v.x1[i], v.y1[i], eps);
    }
    template <class V, class I>
    static AKZ_HD void terms3(const V& v, I i, const double (&c)[4], double s0, double s1, double (&t)[kSums3]) {
        refit_terms3(v.x0[i], v.y0[i], v.x1[i], v.y1[i], c[0], c[1], s0, c[2], c[3], s1, t);
    }
    template <class M>
    static AKZ_HD void normal_matrix(M& m, const double* sums) {
        refit_normal_matrix(m, sums);
    }
    template <class M>
    static AKZ_HD bool model_from_rotated(M& m, double count, float epsilon_model, const double (&c)[4], double s0, double s1, float (&h)[9]) {
        return refit_model_from_rotated(m, count, epsilon_model, c[0], c[1], s0, c[2], c[3], s1, h);
    }
};

}  // namespace akz
