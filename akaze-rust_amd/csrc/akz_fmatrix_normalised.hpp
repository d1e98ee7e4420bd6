// The trial model of the seeded RANSAC's third kind (AKZ_RANSAC_FUNDAMENTAL_NORMALISED; include/akaze_hip.h): the
// Hartley-normalised 8-point algorithm with rank 2 enforced, judged by the Sampson distance in pixels -- as ONE piece of source
// for the host statement (seeded_host, akz_ransac_seeded.cpp; akz_estimate_fundamental_normalised) and the device kernels
// (k_seeded_round<FundamentalNormalisedDev, NW>, akz_ransac_kernels.hip), like akz_fmatrix.hpp for the reference's model: f64
// in a fixed order, no contraction, the same bits on both sides.
//
// The model of a sample IS fit(S) of akz_fundamental_refit.hpp with |S| = 8 -- its functions are called, not restated: passes 1
// and 2 (refit_terms1, refit_terms2, refit_scale), the 36 sums of fund_refit_terms3, fund_refit_normal_matrix, the nine-row
// sweeps and fund_refit_model_from_rotated with count 8 and AKZ_FUNDAMENTAL_REFIT_EPSILON.  That header's note argues why A^T A
// is safe on normalised coordinates, with sets of 8 points as its worst case.
// Every sum over the eight elements e0 .. e7 (the sample in ascending index order) is
//     ((p0 + p2) + (p1 + p3)),  p_j = (0.0 + e_j) + (0.0 + e_{j+4})
// which is what the refit's 256-lane tree does to eight members in lanes 0 .. 7.  So the model of a sample equals one fit of
// akz_refine_fundamental_matrix over the same eight matches, bit for bit.  (The device forms p_j on lane j of the trial's four
// and combines by two exchanges; IEEE addition commutes, so the four lanes hold the same bits.)
// No model: a mean distance of 0 in either image, the rank rule, a norm that is zero or not finite -- the refit's rules.
//
// The inlier rule (sampson_inlier): the first-order geometric (Sampson) distance below eps pixels, without a division, f32 in
// the order written there.  Strict: a zero model or a NaN anywhere passes nothing.
#pragma once
#include "akz_fundamental_refit.hpp"

namespace akz {

// one lane's part of a sum of eight: elements j and j + 4, each from +0.0
AKZ_HD double sum8_part(double a, double b) { return (0.0 + a) + (0.0 + b); }
// the four parts in the tree's order
AKZ_HD double sum8_join(double p0, double p1, double p2, double p3) { return (p0 + p2) + (p1 + p3); }

// F with the convention of fundamental_error (p1^T F p0): s = p1^T F p0, d = |(F p0)_xy|^2 + |(F^T p1)_xy|^2; inlier iff
// s^2 < eps^2 d, i.e. the Sampson distance |s| / sqrt(d) is below eps pixels
AKZ_HD bool sampson_inlier(const float (&f)[9], float x0, float y0, float x1, float y1, float eps) {
    const float l0 = (f[0] * x0 + f[1] * y0) + f[2], l1 = (f[3] * x0 + f[4] * y0) + f[5], l2 = (f[6] * x0 + f[7] * y0) + f[8];
    const float s = (l0 * x1 + l1 * y1) + l2;
    const float m0 = (f[0] * x1 + f[3] * y1) + f[6], m1 = (f[1] * x1 + f[4] * y1) + f[7];
    const float d = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
    return s * s < (eps * eps) * d;
}

// x0, y0 from keypoints_0 and x1, y1 from keypoints_1 of the eight sampled matches (ascending) -> the model, row-major
AKZ_HD bool fundamental_normalised_from_8(const float (&x0)[8], const float (&y0)[8], const float (&x1)[8], const float (&y1)[8],
                                          float epsilon, float (&f)[9]) {
    double p1[4][4], p2[4][2], p3[4][kFundRefitSums3];
    for (int j = 0; j < 4; ++j) {
        double a[4], b[4];
        refit_terms1(x0[j], y0[j], x1[j], y1[j], a);
        refit_terms1(x0[j + 4], y0[j + 4], x1[j + 4], y1[j + 4], b);
        for (int k = 0; k < 4; ++k) p1[j][k] = sum8_part(a[k], b[k]);
    }
    double c[4];
    for (int k = 0; k < 4; ++k) c[k] = sum8_join(p1[0][k], p1[1][k], p1[2][k], p1[3][k]) / 8.0;
    for (int j = 0; j < 4; ++j) {
        double a[2], b[2];
        refit_terms2(x0[j], y0[j], x1[j], y1[j], c[0], c[1], c[2], c[3], a);
        refit_terms2(x0[j + 4], y0[j + 4], x1[j + 4], y1[j + 4], c[0], c[1], c[2], c[3], b);
        for (int k = 0; k < 2; ++k) p2[j][k] = sum8_part(a[k], b[k]);
    }
    double s0 = 0.0, s1 = 0.0;
    if (!refit_scale(sum8_join(p2[0][0], p2[1][0], p2[2][0], p2[3][0]), 8.0, s0) ||
        !refit_scale(sum8_join(p2[0][1], p2[1][1], p2[2][1], p2[3][1]), 8.0, s1))
        return false;
    for (int j = 0; j < 4; ++j) {
        double a[kFundRefitSums3], b[kFundRefitSums3];
        fund_refit_terms3(x0[j], y0[j], x1[j], y1[j], c[0], c[1], s0, c[2], c[3], s1, a);
        fund_refit_terms3(x0[j + 4], y0[j + 4], x1[j + 4], y1[j + 4], c[0], c[1], s0, c[2], c[3], s1, b);
        for (int k = 0; k < kFundRefitSums3; ++k) p3[j][k] = sum8_part(a[k], b[k]);
    }
    double sums[kFundRefitSums3];
    for (int k = 0; k < kFundRefitSums3; ++k) sums[k] = sum8_join(p3[0][k], p3[1][k], p3[2][k], p3[3][k]);
    Mat9x9 m;
    fund_refit_normal_matrix(m, sums);
    jacobi_sweeps_rows<9>(m);
    return fund_refit_model_from_rotated(m, 8.0, epsilon, c[0], c[1], s0, c[2], c[3], s1, f);
}

// The model as a RANSAC model of the seeded family (seeded_host and the seeded kernels; see FundamentalRansac).  epsilon of
// from_sample is the refit's rank rule (AKZ_FUNDAMENTAL_REFIT_EPSILON); eps of inlier is a distance in pixels.
struct FundamentalNormalisedRansac {
    static constexpr int K = 8;
    static constexpr bool kKeepAllWithoutWinner = false;  // no winner: the zero model is evaluated, and keeps nothing
    static constexpr bool kModelOut = true;
    static constexpr bool kZeroModelOut = true;
    static AKZ_HD bool from_sample(const float (&x0)[8], const float (&y0)[8], const float (&x1)[8], const float (&y1)[8], float epsilon,
                                   float (&f)[9]) {
        return fundamental_normalised_from_8(x0, y0, x1, y1, epsilon, f);
    }
    static AKZ_HD bool inlier(const float (&f)[9], float x0, float y0, float x1, float y1, float eps) {
        return sampson_inlier(f, x0, y0, x1, y1, eps);
    }
};

// FundamentalRefit with that inlier rule (akz_refine_fundamental_normalised, k_refit<FundamentalNormalisedRefit>)
struct FundamentalNormalisedRefit : FundamentalRefit {
    template <class V, class I>
    static AKZ_HD bool inlier(const float (&f)[9], const V& v, I i, float eps) {
#if defined(__HIP_DEVICE_COMPILE__)
        // eps in a vector register, as in FundamentalRefit::inlier and for its reason: this instantiation spilled 22 scalar registers
        // into vector lanes with the rule's uniform operands all held there (the arithmetic is the same)
        asm("" : "+v"(eps));
#endif
        return sampson_inlier(f, v.x0[i], v.y0[i], v.x1[i], v.y1[i], eps);
    }
};

}  // namespace akz
