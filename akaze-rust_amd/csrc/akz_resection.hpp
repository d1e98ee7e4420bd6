// Absolute pose (camera resection) from 2D-3D correspondences, the fourth model of the seeded family (AKZ_RANSAC_RESECTION;
// include/akaze_hip.h) -- as ONE piece of source for the host statement (akz_resection_api.cpp) and the device
// kernels (akz_resection.hip), like akz_fmatrix_normalised.hpp for the third kind: f64 in a fixed order unless stated, no
// contraction (-ffp-contract=off on both sides), the same bits on both sides.
//
// A problem: n correspondences, each a point (X, Y, Z) in f32 and a pixel (u, v) in f32, and one pinhole camera.  The pose is
// x_cam = R X + t.  The camera's four fields are cast to f32 ONCE per problem (res_camera); the fit widens those casts back to
// f64 and the inlier rule works on them as they are -- nothing in the statement sees the f64 fields again.
//
// fit(S) over a set S of correspondences -- the trial model with |S| = 6 (resection_from_6) and the refit's model with S the
// inliers (the host's and the device's 256-lane tree), the same functions called by both:
//   1. a = (u - cx) / fx, b = (v - cy) / fy  (res_terms*: u, v, cx, cy, fx, fy widened first).
//   2. Hartley normalisation of both sides with the refit's pass shapes: pass 1 the sums of a, b, X, Y, Z and the centroids
//      c = sum / |S|; pass 2 the sums of sqrt(da da + db db) and sqrt((dX dX + dY dY) + dZ dZ); the pixels' mean distance goes
//      to sqrt 2 (refit_scale), the points' to sqrt 3 (res_scale3); a mean distance of 0 on either side: no model.
//   3. with (a, b) and Xh = (x, y, z, 1) normalised, q = the ten distinct entries {xx, xy, xz, x, yy, yz, y, zz, z, 1} of
//      Xh Xh^T: the 40 sums of q[k], a q[k], b q[k], (a a + b b) q[k] (sum 10 g + k).  They are the blocks P, Q_a, Q_b, W of the
//      normal matrix M = A^T A of the DLT rows [Xh, 0, -a Xh] and [0, Xh, -b Xh]:
//          M = [[P, 0, -Q_a], [0, P, -Q_b], [-Q_a, -Q_b, W]]   (12 x 12, symmetric, 4 x 4 blocks).
//      Every sum over S runs in the order of the refit's tree (akz_homography_refit.hpp), each element from +0.0; for six
//      members that is sum8_part / sum8_join of akz_fmatrix_normalised.hpp with e6 and e7 absent (a part of one element is
//      (0.0 + e_j) + 0.0).
//   4. null vector: jacobi_sweeps_rows<12, 12> on M (the device: jacobi_sweep_levels<12, 12>); the row of the smallest norm, the
//      first among equals, normalised; every OTHER row norm must exceed eps_m^2 |S| / 6 (eps_m = AKZ_FUNDAMENTAL_REFIT_EPSILON:
//      the refit's rank rule scaled to six points), else no model.  P~ = the vector as a 3 x 4 matrix, row-major.
//   5. P^ = T2^-1 P~ T3 with T3 = [[s3, 0, 0, -s3 cX], .., [0, 0, 0, 1]] and T2^-1 = [[1 / s2, 0, ca], [0, 1 / s2, cb], [0, 0, 1]];
//      P^ = s [R | t].  det of its left block M3 negative: P^ changes sign.  The Hestenes rotations of akz_pose.hpp's
//      decomposition on the three rows of a copy of M3: the rotated rows are sigma_i v_i^T, ordered by norm descending (the first
//      among equals first).  No model if sigma1 is zero or not finite or if !(sigma3 > eps_m sigma1).  u_i = (M3 v_i) / sigma_i;
//      R = U V^T, R[r][c] = (u1[r] v1[c] + u2[r] v2[c]) + u3[r] v3[c] -- the rotation nearest M3 in Frobenius norm, proper because
//      det M3 > 0 --; t = P^[:, 3] / (((sigma1 + sigma2) + sigma3) / 3); both rounded to f32; sigma = {1, sigma2 / sigma1,
//      sigma3 / sigma1} as f32.
// THE sigma3 RULE IS WHAT REFUSES COPLANAR POINTS: the DLT's null space has more than one dimension on a plane, the vector the
// sweeps leave is some member of it, and its M3 is singular up to rounding.  A planar scene needs another solver; this one
// answers found = 0 on it.
// Forming A^T A squares the condition number (see the note in akz_fundamental_refit.hpp); on normalised coordinates the eleven
// non-zero singular values of A on six points in general position lie within ~1e4 of each other, so the squared 1e8 leaves
// seven to eight digits in f64 for a result rounded to f32.  Samples nearer to degenerate than that are noise to RANSAC anyway.
//
// The inlier rule (res_inlier), f32 in this order, no division:
//     c_r = ((R[r][0] X + R[r][1] Y) + R[r][2] Z) + t[r],  r = 0, 1, 2
//     ex = fx c_0 - (u - cx) c_2;   ey = fy c_1 - (v - cy) c_2
//     inlier iff c_2 > 0 and ex ex + ey ey < (eps eps) (c_2 c_2)
// with fx, fy, cx, cy the f32 casts.  eps is in pixels (for fx = fy; else the error ellipse of the two focal lengths), the test
// is strict, and a NaN anywhere passes nothing -- so neither does the zero model.
//
// A model is 15 floats: r (9, row-major) | t (3) | sigma (3).
#pragma once
#include <cstdint>

#include "../../include/akaze_hip.h"
#include "akz_fmatrix_normalised.hpp"  // sum8_part, sum8_join
#include "akz_pose.hpp"                // pose_dot3, pose_finite

namespace akz {

constexpr int kResK = 6;              // correspondences per sample, and the least a problem runs on
constexpr int kResRows = 12;          // rows and columns of M
constexpr int kResSums1 = 5;          // sums of pass 1
constexpr int kResSums3 = 40;         // sums of pass 3
constexpr int kResModelFloats = 15;   // r | t | sigma

struct ResCamera {
    float fx, fy, cx, cy;
};
AKZ_HD ResCamera res_camera(const akz_camera& k) { return ResCamera{(float)k.fx, (float)k.fy, (float)k.cx, (float)k.cy}; }

struct Mat12x12 {
    double v[kResRows][kResRows];
    AKZ_HD double& at(int p, int k) { return v[p][k]; }
};

// t = {a, b, X, Y, Z}
AKZ_HD void res_terms1(float X, float Y, float Z, float u, float v, const ResCamera& k, double (&t)[kResSums1]) {
    t[0] = ((double)u - (double)k.cx) / (double)k.fx;
    t[1] = ((double)v - (double)k.cy) / (double)k.fy;
    t[2] = (double)X;
    t[3] = (double)Y;
    t[4] = (double)Z;
}
// t = {|(a, b) - c|, |(X, Y, Z) - c|}
AKZ_HD void res_terms2(float X, float Y, float Z, float u, float v, const ResCamera& k, const double (&c)[kResSums1], double (&t)[2]) {
    double e[kResSums1];
    res_terms1(X, Y, Z, u, v, k, e);
    const double da = e[0] - c[0], db = e[1] - c[1], dx = e[2] - c[2], dy = e[3] - c[3], dz = e[4] - c[4];
    t[0] = sqrt(da * da + db * db);
    t[1] = sqrt((dx * dx + dy * dy) + dz * dz);
}
// refit_scale for three dimensions: the mean distance goes to sqrt 3
AKZ_HD bool res_scale3(double sum_d, double count, double& s) {
    const double d = sum_d / count;
    if (!(d > 0.0)) return false;
    s = 1.7320508075688772 / d;  // sqrt(3) / d
    return true;
}
// t[k] = q[k], t[10 + k] = a q[k], t[20 + k] = b q[k], t[30 + k] = (a a + b b) q[k]
AKZ_HD void res_terms3(float X, float Y, float Z, float u, float v, const ResCamera& k, const double (&c)[kResSums1], double s2, double s3,
                       double (&t)[kResSums3]) {
    double e[kResSums1];
    res_terms1(X, Y, Z, u, v, k, e);
    const double a = s2 * (e[0] - c[0]), b = s2 * (e[1] - c[1]);
    const double x = s3 * (e[2] - c[2]), y = s3 * (e[3] - c[3]), z = s3 * (e[4] - c[4]);
    const double q[10] = {x * x, x * y, x * z, x, y * y, y * z, y, z * z, z, 1.0};
    const double w = a * a + b * b;
    AKZ_UNROLL
    for (int j = 0; j < 10; ++j) {
        t[j] = q[j];
        t[10 + j] = a * q[j];
        t[20 + j] = b * q[j];
        t[30 + j] = w * q[j];
    }
}
// index of (i, j) among the ten distinct entries of a symmetric 4 x 4, row by row from the diagonal
AKZ_HD int res_sym_index(int i, int j) {
    const int lo = i <= j ? i : j, hi = i <= j ? j : i;
    return lo == 0 ? hi : (lo == 1 ? 3 + hi : (lo == 2 ? 5 + hi : 9));
}
// M (12 x 12) from the 40 sums of pass 3
template <class M>
AKZ_HD void res_normal_matrix(M& m, const double* sums) {
    AKZ_UNROLL
    for (int i = 0; i < 4; ++i) {
        AKZ_UNROLL
        for (int j = 0; j < 4; ++j) {
            const int k = res_sym_index(i, j);
            const double p = sums[k], qa = sums[10 + k], qb = sums[20 + k], w = sums[30 + k];
            m.at(i, j) = p;
            m.at(i, 4 + j) = 0.0;
            m.at(i, 8 + j) = -qa;
            m.at(4 + i, j) = 0.0;
            m.at(4 + i, 4 + j) = p;
            m.at(4 + i, 8 + j) = -qb;
            m.at(8 + i, j) = -qa;
            m.at(8 + i, 4 + j) = -qb;
            m.at(8 + i, 8 + j) = w;
        }
    }
}

// the model from the rotated M (after the sweeps) and the normalisation: steps 4 (from the smallest row on) and 5; count = |S|.
// Rows 0 .. 2 of m are overwritten (the 3 x 3 matrix of step 5 in their first three columns).
template <class M>
AKZ_HD bool res_model_from_rotated(M& m, double count, float epsilon_model, const double (&c)[kResSums1], double s2, double s3,
                                   float (&mdl)[kResModelFloats]) {
    int mi = 0;
    double smallest = 0.0;
    AKZ_NOUNROLL
    for (int i = 0; i < kResRows; ++i) {
        double nrm = 0.0;
        AKZ_UNROLL
        for (int k = 0; k < kResRows; ++k) nrm += m.at(i, k) * m.at(i, k);
        nrm = sqrt(nrm);
        if (i == 0 || nrm < smallest) {  // the first one among equals
            smallest = nrm;
            mi = i;
        }
    }
    const double threshold = ((double)epsilon_model * (double)epsilon_model) * (count / 6.0);
    bool full = true;
    AKZ_NOUNROLL
    for (int i = 0; i < kResRows; ++i) {
        double nrm = 0.0;
        AKZ_UNROLL
        for (int k = 0; k < kResRows; ++k) nrm += m.at(i, k) * m.at(i, k);
        nrm = sqrt(nrm);
        if (i != mi && !(nrm > threshold)) full = false;
    }
    if (!full) return false;
    double ph[12];  // P~, row-major 3 x 4
    AKZ_UNROLL
    for (int k = 0; k < 12; ++k) ph[k] = smallest > 0.0 ? m.at(mi, k) / smallest : 0.0;
    // B = P~ T3
    const double tx = -(s3 * c[2]), ty = -(s3 * c[3]), tz = -(s3 * c[4]);
    double bm[12];
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        bm[4 * r + 0] = ph[4 * r + 0] * s3;
        bm[4 * r + 1] = ph[4 * r + 1] * s3;
        bm[4 * r + 2] = ph[4 * r + 2] * s3;
        bm[4 * r + 3] = ((ph[4 * r + 0] * tx + ph[4 * r + 1] * ty) + ph[4 * r + 2] * tz) + ph[4 * r + 3];
    }
    // P^ = T2^-1 B
    double pm[12];
    AKZ_UNROLL
    for (int k = 0; k < 4; ++k) {
        pm[k] = bm[k] / s2 + c[0] * bm[8 + k];
        pm[4 + k] = bm[4 + k] / s2 + c[1] * bm[8 + k];
        pm[8 + k] = bm[8 + k];
    }
    const double det = (pm[0] * (pm[5] * pm[10] - pm[6] * pm[9]) - pm[1] * (pm[4] * pm[10] - pm[6] * pm[8])) +
                       pm[2] * (pm[4] * pm[9] - pm[5] * pm[8]);
    if (det < 0.0) {
        AKZ_UNROLL
        for (int k = 0; k < 12; ++k) pm[k] = -pm[k];
    }
    const double m3[9] = {pm[0], pm[1], pm[2], pm[4], pm[5], pm[6], pm[8], pm[9], pm[10]};
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        AKZ_UNROLL
        for (int k = 0; k < 3; ++k) m.at(r, k) = m3[3 * r + k];
    }
    jacobi_sweeps_rows<3, 3>(m);
    double nrm[3];
    AKZ_UNROLL
    for (int i = 0; i < 3; ++i) nrm[i] = sqrt((m.at(i, 0) * m.at(i, 0) + m.at(i, 1) * m.at(i, 1)) + m.at(i, 2) * m.at(i, 2));
    // (the order of pose_decompose: the largest, the first among equals; then the larger of the two others)
    int i1 = 0;
    double g1 = nrm[0];
    if (nrm[1] > g1) i1 = 1, g1 = nrm[1];
    if (nrm[2] > g1) i1 = 2, g1 = nrm[2];
    const int ja = i1 == 0 ? 1 : 0, jb = i1 == 2 ? 1 : 2;  // the two others, ascending
    const double na = i1 == 0 ? nrm[1] : nrm[0], nb = i1 == 2 ? nrm[1] : nrm[2];
    const int i2 = nb > na ? jb : ja, i3 = nb > na ? ja : jb;
    const double g2 = nb > na ? nb : na, g3 = nb > na ? na : nb;
    if (!(g1 > 0.0) || !pose_finite(g1)) return false;
    if (!(g3 > (double)epsilon_model * g1)) return false;
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
    AKZ_UNROLL
    for (int k = 0; k < 3; ++k) {
        v1[k] = m.at(i1, k) / g1;
        v2[k] = m.at(i2, k) / g2;
        v3[k] = m.at(i3, k) / g3;
    }
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        u1[r] = pose_dot3(m3 + 3 * r, v1) / g1;
        u2[r] = pose_dot3(m3 + 3 * r, v2) / g2;
        u3[r] = pose_dot3(m3 + 3 * r, v3) / g3;
    }
    const double scale = ((g1 + g2) + g3) / 3.0;
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        AKZ_UNROLL
        for (int k = 0; k < 3; ++k) mdl[3 * r + k] = (float)((u1[r] * v1[k] + u2[r] * v2[k]) + u3[r] * v3[k]);
        mdl[9 + r] = (float)(pm[4 * r + 3] / scale);
    }
    mdl[12] = 1.0f;
    mdl[13] = (float)(g2 / g1);
    mdl[14] = (float)(g3 / g1);
    return true;
}

AKZ_HD bool res_inlier(const float (&m)[kResModelFloats], const ResCamera& k, float X, float Y, float Z, float u, float v, float eps) {
    const float c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[9];
    const float c1 = ((m[3] * X + m[4] * Y) + m[5] * Z) + m[10];
    const float c2 = ((m[6] * X + m[7] * Y) + m[8] * Z) + m[11];
    const float ex = k.fx * c0 - (u - k.cx) * c2, ey = k.fy * c1 - (v - k.cy) * c2;
    return c2 > 0.0f && ex * ex + ey * ey < (eps * eps) * (c2 * c2);
}

// The resection as a refit model (the concept: akz_homography_refit.hpp), for refit_loop_host and the device's refit_loop.  A view:
// X[i] .. v[i] of the problem's correspondences and its camera `cam`.
struct ResectionRefit {
    static constexpr int kMin = kResK, kSums1 = kResSums1, kSums3 = kResSums3, kRows = kResRows, kFloats = kResModelFloats;
    using Mat = Mat12x12;
    template <class V, class I>
    static AKZ_HD bool inlier(const float (&m)[kFloats], const V& q, I i, float eps) {
        return res_inlier(m, q.cam, q.X[i], q.Y[i], q.Z[i], q.u[i], q.v[i], eps);
    }
    template <class V, class I>
    static AKZ_HD void terms1(const V& q, I i, double (&t)[kSums1]) {
        res_terms1(q.X[i], q.Y[i], q.Z[i], q.u[i], q.v[i], q.cam, t);
    }
    template <class V, class I>
    static AKZ_HD void terms2(const V& q, I i, const double (&c)[kSums1], double (&t)[2]) {
        res_terms2(q.X[i], q.Y[i], q.Z[i], q.u[i], q.v[i], q.cam, c, t);
    }
    static AKZ_HD bool scale2(double sum_d, double count, double& s) { return res_scale3(sum_d, count, s); }
    template <class V, class I>
    static AKZ_HD void terms3(const V& q, I i, const double (&c)[kSums1], double s2, double s3, double (&t)[kSums3]) {
        res_terms3(q.X[i], q.Y[i], q.Z[i], q.u[i], q.v[i], q.cam, c, s2, s3, t);
    }
    template <class M>
    static AKZ_HD void normal_matrix(M& m, const double* sums) {
        res_normal_matrix(m, sums);
    }
    template <class M>
    static AKZ_HD bool model_from_rotated(M& m, double count, float epsilon_model, const double (&c)[kSums1], double s2, double s3,
                                          float (&mdl)[kFloats]) {
        return res_model_from_rotated(m, count, epsilon_model, c, s2, s3, mdl);
    }
};

// The model of one sample: six correspondences in ascending order of their position in the problem.  Part j of a sum holds
// elements j and j + 4; parts 2 and 3 have no second element.
AKZ_HD bool resection_from_6(const float (&X)[kResK], const float (&Y)[kResK], const float (&Z)[kResK], const float (&u)[kResK],
                             const float (&v)[kResK], const ResCamera& k, float epsilon, float (&mdl)[kResModelFloats]) {
    double p1[4][kResSums1], p2[4][2], p3[4][kResSums3];
    for (int j = 0; j < 4; ++j) {
        double a[kResSums1], b[kResSums1] = {};
        res_terms1(X[j], Y[j], Z[j], u[j], v[j], k, a);
        if (j < 2) res_terms1(X[j + 4], Y[j + 4], Z[j + 4], u[j + 4], v[j + 4], k, b);
        for (int i = 0; i < kResSums1; ++i) p1[j][i] = sum8_part(a[i], j < 2 ? b[i] : 0.0);
    }
    double c[kResSums1];
    for (int i = 0; i < kResSums1; ++i) c[i] = sum8_join(p1[0][i], p1[1][i], p1[2][i], p1[3][i]) / 6.0;
    for (int j = 0; j < 4; ++j) {
        double a[2], b[2] = {};
        res_terms2(X[j], Y[j], Z[j], u[j], v[j], k, c, a);
        if (j < 2) res_terms2(X[j + 4], Y[j + 4], Z[j + 4], u[j + 4], v[j + 4], k, c, b);
        for (int i = 0; i < 2; ++i) p2[j][i] = sum8_part(a[i], j < 2 ? b[i] : 0.0);
    }
    double s2 = 0.0, s3 = 0.0;
    if (!refit_scale(sum8_join(p2[0][0], p2[1][0], p2[2][0], p2[3][0]), 6.0, s2) ||
        !res_scale3(sum8_join(p2[0][1], p2[1][1], p2[2][1], p2[3][1]), 6.0, s3))
        return false;
    for (int j = 0; j < 4; ++j) {
        double a[kResSums3], b[kResSums3] = {};
        res_terms3(X[j], Y[j], Z[j], u[j], v[j], k, c, s2, s3, a);
        if (j < 2) res_terms3(X[j + 4], Y[j + 4], Z[j + 4], u[j + 4], v[j + 4], k, c, s2, s3, b);
        for (int i = 0; i < kResSums3; ++i) p3[j][i] = sum8_part(a[i], j < 2 ? b[i] : 0.0);
    }
    double sums[kResSums3];
    for (int i = 0; i < kResSums3; ++i) sums[i] = sum8_join(p3[0][i], p3[1][i], p3[2][i], p3[3][i]);
    Mat12x12 m;
    res_normal_matrix(m, sums);
    jacobi_sweeps_rows<kResRows, kResRows>(m);
    return res_model_from_rotated(m, 6.0, epsilon, c, s2, s3, mdl);
}

}  // namespace akz
