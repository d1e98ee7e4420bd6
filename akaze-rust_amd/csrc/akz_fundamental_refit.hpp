// Local optimisation of the winning fundamental matrix: the least-squares refit on its inliers and the re-classification, as
// ONE piece of source for the host statement (akz_refine_fundamental_matrix, akz_ransac.cpp) and the device kernel
// (k_refit<FundamentalRefit>, akz_homography_refit.hip), like akz_homography_refit.hpp for the homography: f64 in a fixed
// order, no contraction, the same bits on both sides.
//
// The loop is the one of akz_homography_refit.hpp, unchanged (S, fit, reclassify, reject if smaller, stop when not grown),
// over the pair's RAW list, with the inlier rule of the RANSAC itself: fundamental_error(f, ..) < epsilon_inlier.  So the
// result never has fewer inliers than the input.
//
// fit(S), |S| >= 8 (fewer: no model).  Every sum over S is formed in the order of akz_homography_refit.hpp (element i in lane
// i mod 256, ascending from +0.0, then the tree s = 128 .. 1):
//   1., 2. Hartley normalisation of both images: passes 1 and 2 of the homography refit (refit_terms1, refit_terms2,
//      refit_scale); d == 0 in either image: no model.
//   3. with p = (x, y, 1) and q = (u, v, 1) in normalised coordinates, a = {x x, x y, x, y y, y, 1} and b the same six products
//      of q: the 36 sums of a[k] b[l] (sum 6 k + l).  They are every entry of the 9 x 9 normal matrix M = A^T A of the design
//      rows of design_row (akz_fmatrix.hpp), whose entry 3 i + j is p_i q_j:  M[3 i + j][3 k + l] = sum p_i p_k q_j q_l.
//   4. null vector: jacobi_sweeps_rows<9> on M (the device: jacobi_sweep_levels<9>).  The rotated rows are lambda_i v_i^T; the
//      row of the smallest norm (the first among equals) is the one of the null vector.  Rank rule: every OTHER row norm must
//      exceed eps_m^2 |S| / 8 (eps_m = AKZ_FUNDAMENTAL_REFIT_EPSILON: the homography's rule scaled to 8 points), else no model.
//      That row, normalised, is v (a zero row: v = 0, and the norm rule of 6. refuses the model); F^ is formed from v as
//      model_from_rotated forms the trial model, F^[j][i] = v[3 i + j], but stays in f64.
//      The sweeps stop when every pair of rows is orthogonal RELATIVE to the two norms, so the smallest row is orthogonal to
//      the eight others however small it is: its direction is the null vector's even for exact data (lambda_9 ~ 0).
//   5. rank 2: the same Hestenes rotations on the three rows of a copy of F^ (a 3 x 9 matrix whose columns 3 .. 8 are zero:
//      jacobi_sweeps_rows<3>).  r = the row of the smallest norm after the sweeps (the first among equals) is sigma_3 times the
//      third right singular vector.  |r| > 0: v3 = r / |r| and F' = F^ - (F^ v3) v3^T; else F' = F^.
//   6. F = T1^T F' T0 with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], scaled to unit Frobenius norm (the trial models have
//      it, and epsilon_inlier only means anything at that scale), rounded to f32.  A norm that is zero or not finite: no model.
// Forming A^T A squares the condition number (see the note in akz_fmatrix.hpp).  On Hartley-normalised points the entries of a
// design row are products of coordinates of size ~1 and the eight non-zero singular values of A lie within 3e1 .. 6e3 of each
// other (the largest on sets of 8 points; 3e1 .. 7e1 from 255 points on), so the squared 4e7 at most leaves eight digits in
// f64 for a result that is rounded to f32: harmless here, unlike the raw pixel coordinates (entries of ~1e6) that the trial
// model works on and that note speaks of.
#pragma once
#include "akz_homography_refit.hpp"

namespace akz {

constexpr int kFundRefitSums3 = 36;  // sums of pass 3

// index of (i, j) among the six distinct entries {00, 01, 02, 11, 12, 22} of a symmetric 3 x 3
AKZ_HD int refit_sym_index(int i, int j) {
    return i <= j ? (i == 0 ? j : (i == 1 ? 2 + j : 5)) : (j == 0 ? i : (j == 1 ? 2 + i : 5));
}

// t[6 k + l] = a[k] b[l]
AKZ_HD void fund_refit_terms3(float x0, float y0, float x1, float y1, double c0x, double c0y, double s0, double c1x, double c1y, double s1,
                              double (&t)[kFundRefitSums3]) {
    const double x = s0 * ((double)x0 - c0x), y = s0 * ((double)y0 - c0y);
    const double u = s1 * ((double)x1 - c1x), v = s1 * ((double)y1 - c1y);
    const double a[6] = {x * x, x * y, x, y * y, y, 1.0};
    const double b[6] = {u * u, u * v, u, v * v, v, 1.0};
    AKZ_UNROLL
    for (int k = 0; k < 6; ++k) {
        AKZ_UNROLL
        for (int l = 0; l < 6; ++l) t[6 * k + l] = a[k] * b[l];
    }
}

// M (9 x 9) from the 36 sums of pass 3
template <class M>
AKZ_HD void fund_refit_normal_matrix(M& m, const double* sums) {
    AKZ_UNROLL
    for (int r = 0; r < 9; ++r) {
        AKZ_UNROLL
        for (int c = 0; c < 9; ++c) m.at(r, c) = sums[6 * refit_sym_index(r / 3, c / 3) + refit_sym_index(r % 3, c % 3)];
    }
}

// the model from the rotated M (after the sweeps) and the normalisation: steps 4 (from the smallest row on), 5 and 6; count =
// |S|.  Rows 0 .. 2 of m are overwritten (the 3 x 9 matrix of step 5).
template <class M>
AKZ_HD bool fund_refit_model_from_rotated(M& m, double count, float epsilon_model, double c0x, double c0y, double s0, double c1x, double c1y,
                                          double s1, float (&f)[9]) {
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
    const double threshold = ((double)epsilon_model * (double)epsilon_model) * (count * 0.125);
    bool full = true;
    AKZ_NOUNROLL
    for (int i = 0; i < 9; ++i) {
        double nrm = 0.0;
        AKZ_UNROLL
        for (int k = 0; k < 9; ++k) nrm += m.at(i, k) * m.at(i, k);
        nrm = sqrt(nrm);
        if (i != mi && !(nrm > threshold)) full = false;
    }
    if (!full) return false;
    double v[9];
    AKZ_UNROLL
    for (int k = 0; k < 9; ++k) v[k] = smallest > 0.0 ? m.at(mi, k) / smallest : 0.0;
    const double fh[9] = {v[0], v[3], v[6], v[1], v[4], v[7], v[2], v[5], v[8]};
    // rank 2
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        AKZ_UNROLL
        for (int k = 0; k < 9; ++k) m.at(r, k) = k < 3 ? fh[3 * r + k] : 0.0;
    }
    jacobi_sweeps_rows<3>(m);
    int ri = 0;
    double rn = 0.0;
    AKZ_NOUNROLL
    for (int i = 0; i < 3; ++i) {
        double nrm = 0.0;
        AKZ_UNROLL
        for (int k = 0; k < 3; ++k) nrm += m.at(i, k) * m.at(i, k);
        nrm = sqrt(nrm);
        if (i == 0 || nrm < rn) {
            rn = nrm;
            ri = i;
        }
    }
    double f2[9];
    if (rn > 0.0) {
        const double v3[3] = {m.at(ri, 0) / rn, m.at(ri, 1) / rn, m.at(ri, 2) / rn};
        AKZ_UNROLL
        for (int r = 0; r < 3; ++r) {
            const double d = (fh[3 * r] * v3[0] + fh[3 * r + 1] * v3[1]) + fh[3 * r + 2] * v3[2];
            AKZ_UNROLL
            for (int k = 0; k < 3; ++k) f2[3 * r + k] = fh[3 * r + k] - d * v3[k];
        }
    } else {
        AKZ_UNROLL
        for (int k = 0; k < 9; ++k) f2[k] = fh[k];
    }
    // A = F' T0
    const double tx0 = -(s0 * c0x), ty0 = -(s0 * c0y), tx1 = -(s1 * c1x), ty1 = -(s1 * c1y);
    double a[9];
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        a[3 * r + 0] = f2[3 * r + 0] * s0;
        a[3 * r + 1] = f2[3 * r + 1] * s0;
        a[3 * r + 2] = (f2[3 * r + 0] * tx0 + f2[3 * r + 1] * ty0) + f2[3 * r + 2];
    }
    // F = T1^T A with T1^T = [[s1, 0, 0], [0, s1, 0], [-s1 c1x, -s1 c1y, 1]]
    double F[9];
    AKZ_UNROLL
    for (int col = 0; col < 3; ++col) {
        F[col] = s1 * a[col];
        F[3 + col] = s1 * a[3 + col];
        F[6 + col] = (tx1 * a[col] + ty1 * a[3 + col]) + a[6 + col];
    }
    double fro = 0.0;
    AKZ_UNROLL
    for (int j = 0; j < 9; ++j) fro += F[j] * F[j];
    fro = sqrt(fro);
    if (!(fro > 0.0) || !(fro <= 1.7976931348623157e308)) return false;  // zero, infinite or NaN
    AKZ_UNROLL
    for (int j = 0; j < 9; ++j) f[j] = (float)(F[j] / fro);
    return true;
}

// The fundamental matrix as a refit model (see TwoViewRefit)
struct FundamentalRefit : TwoViewRefit {
    static constexpr int kMin = 8;
    static constexpr int kSums3 = kFundRefitSums3;
    template <class V, class I>
    static AKZ_HD bool inlier(const float (&f)[9], const V& v, I i, float eps) {
#if defined(__HIP_DEVICE_COMPILE__)
        // eps in a vector register: k_refit<FundamentalRefit> sits at the limit of the scalar registers, and with the rule's uniform
        // operands all held there it spilled 22 of them into vector lanes and two vector registers to scratch (the same arithmetic)
        asm("" : "+v"(eps));
#endif
        return fundamental_error(f, v.x0[i], v.y0[i], v.x1[i], v.y1[i]) < eps;
    }
    template <class V, class I>
    static AKZ_HD void terms3(const V& v, I i, const double (&c)[4], double s0, double s1, double (&t)[kSums3]) {
        fund_refit_terms3(v.x0[i], v.y0[i], v.x1[i], v.y1[i], c[0], c[1], s0, c[2], c[3], s1, t);
    }
    template <class M>
    static AKZ_HD void normal_matrix(M& m, const double* sums) {
        fund_refit_normal_matrix(m, sums);
    }
    template <class M>
    static AKZ_HD bool model_from_rotated(M& m, double count, float epsilon_model, const double (&c)[4], double s0, double s1, float (&f)[9]) {
        return fund_refit_model_from_rotated(m, count, epsilon_model, c[0], c[1], s0, c[2], c[3], s1, f);
    }
};

}  // namespace akz
