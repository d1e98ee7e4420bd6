// The model of one RANSAC trial -- estimate_fundamental_matrix (akaze/src/ops/estimate_fundamental_matrix.rs:17-69) for
// exactly eight correspondences -- as ONE piece of source for the host path (akz_ransac.cpp) and for the device kernel
// that runs the trials of match_features (akz_ransac_kernels.hip): f64 additions, multiplications, divisions and square roots in
// a fixed order, no contraction (-ffp-contract=off on both sides), so that the two produce the same bits.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define AKZ_HD __host__ __device__ inline
#define AKZ_UNROLL _Pragma("unroll")  // (static indices: the device keeps the 8 x 9 matrix in registers)
#else
#define AKZ_HD inline
#define AKZ_UNROLL
#endif

namespace akz {

// Thin SVD of the 8x9 design matrix A by one-sided (Hestenes) Jacobi rotations on the columns of A^T (f64; m[p] is column
// p of A^T, i.e. row p of A): the rotated columns become orthogonal, their norms are the 8 singular values and the
// normalised columns the right singular vectors of A.  Works on A itself, not on A^T A, so the condition number is not
// squared (pixel coordinates of ~1e3 give entries of ~1e6: the eigenvalue route lost the smallest singular values in
// rounding noise).
// The matrix's storage is the caller's (M: double& at(p, k)): an array on the host, LDS on the device.
struct Mat8x9 {
    double v[8][9];
    AKZ_HD double& at(int p, int k) { return v[p][k]; }
};
// one Hestenes rotation of rows p, q (columns of A^T) over their first COLS entries; false: the pair is orthogonal already
// (COLS: nine for every model of two views; the resection of akz_resection.hpp has twelve)
template <int COLS = 9, class M>
AKZ_HD bool jacobi_pair(M& m, int p, int q) {
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
    AKZ_UNROLL
    for (int k = 0; k < COLS; ++k) {
        const double x = m.at(p, k), y = m.at(q, k);
        alpha += x * x;
        beta += y * y;
        gamma += x * y;
    }
    if (fabs(gamma) <= 1e-15 * sqrt(alpha * beta) || gamma == 0.0) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
    AKZ_UNROLL
    for (int k = 0; k < COLS; ++k) {
        const double x = m.at(p, k), y = m.at(q, k);
        m.at(p, k) = c * x - sn * y;
        m.at(q, k) = sn * x + c * y;
    }
    return true;
}
// sweeps over the pairs of the first ROWS rows in row-cyclic order (0,1) (0,2) .. (0,ROWS-1) (1,2) .. until one leaves every
// pair alone
template <int ROWS, int COLS = 9, class M>
AKZ_HD void jacobi_sweeps_rows(M& m) {
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < ROWS; ++p)
            for (int q = p + 1; q < ROWS; ++q) rotated = jacobi_pair<COLS>(m, p, q) || rotated;
        if (!rotated) break;
    }
}
// the 8 x 9 design matrices of the trial models
template <class M>
AKZ_HD void jacobi_sweeps(M& m) {
    jacobi_sweeps_rows<8>(m);
}
// after the sweeps: index of the smallest singular value (row norm); *full_rank = all eight exceed epsilon (as f32)
template <class M>
AKZ_HD int smallest_singular(M& m, float epsilon, bool* full_rank) {
    int rank = 0, mi = 0;
    double smallest = 0.0;
    for (int i = 0; i < 8; ++i) {
        double nrm = 0.0;
        AKZ_UNROLL
        for (int k = 0; k < 9; ++k) nrm += m.at(i, k) * m.at(i, k);
        nrm = sqrt(nrm);
        if ((float)nrm > epsilon) ++rank;
        if (i == 0 || nrm < smallest) {  // the smallest of the 8 (the first one among equals)
            smallest = nrm;
            mi = i;
        }
    }
    *full_rank = rank == 8;
    return mi;
}

// the design matrix of eight correspondences (:26-40), products in f32 as the reference forms them
// (row i of one correspondence: the batched trials of akz_ransac_kernels.hip form the rows of a matrix on several lanes)
template <class M>
AKZ_HD void design_row(M& m, int i, float x0, float y0, float x1, float y1) {
    const float row[9] = {x0 * x1, x0 * y1, x0, y0 * x1, y0 * y1, y0, x1, y1, 1.0f};
    AKZ_UNROLL
    for (int k = 0; k < 9; ++k) m.at(i, k) = (double)row[k];
}
template <class M>
AKZ_HD void design_matrix(M& m, const float (&x0)[8], const float (&y0)[8], const float (&x1)[8], const float (&y1)[8]) {
    for (int i = 0; i < 8; ++i) design_row(m, i, x0[i], y0[i], x1[i], y1[i]);
}
// the model from the rotated matrix: the right singular vector of the smallest of the 8 singular values, as
// [[v0, v3, v6], [v1, v4, v7], [v2, v5, v8]] (:46-66).  false: rank < 8 at `epsilon` (the reference's None, :44).
template <class M>
AKZ_HD bool model_from_rotated(M& m, float epsilon, float (&f)[9]) {
    bool full = false;
    const int mi = smallest_singular(m, epsilon, &full);
    if (!full) return false;
    double nrm = 0.0;
    AKZ_UNROLL
    for (int k = 0; k < 9; ++k) nrm += m.at(mi, k) * m.at(mi, k);
    nrm = sqrt(nrm);
    float v[9];
    AKZ_UNROLL
    for (int k = 0; k < 9; ++k) v[k] = (float)(nrm > 0.0 ? m.at(mi, k) / nrm : 0.0);
    f[0] = v[0]; f[1] = v[3]; f[2] = v[6];
    f[3] = v[1]; f[4] = v[4]; f[5] = v[7];
    f[6] = v[2]; f[7] = v[5]; f[8] = v[8];
    return true;
}

// x0, y0 from keypoints_0 and x1, y1 from keypoints_1 of the eight sampled matches -> the model, row-major
AKZ_HD bool fundamental_from_8(const float (&x0)[8], const float (&y0)[8], const float (&x1)[8], const float (&y1)[8], float epsilon,
                               float (&f)[9]) {
    Mat8x9 m;
    design_matrix(m, x0, y0, x1, y1);
    jacobi_sweeps(m);
    return model_from_rotated(m, epsilon, f);
}

// evaluate_model (:79-83): |p_r^T F p_l| with p_l = (x0, y0, 1), p_r = (x1, y1, 1); the products with 1 are exact
AKZ_HD float fundamental_error(const float (&f)[9], float x0, float y0, float x1, float y1) {
    const float r0 = (x1 * f[0] + y1 * f[3]) + f[6], r1 = (x1 * f[1] + y1 * f[4]) + f[7], r2 = (x1 * f[2] + y1 * f[5]) + f[8];
    const float s = (r0 * x0 + r1 * y0) + r2;
    return fabsf(s);
}

// The fundamental matrix as a RANSAC model, for ransac_host (akz_ransac.cpp) and the kernels of akz_ransac_kernels.hip alike
struct FundamentalRansac {
    static constexpr int K = 8;                           // matches per sample, and the least a call works on
    static constexpr bool kKeepAllWithoutWinner = false;  // no trial with an inlier: the zero model is evaluated (error 0)
    static constexpr bool kModelOut = false;              // the call hands back no model
    static constexpr bool kZeroModelOut = false;          // (with kModelOut: zeros are written where there is no winner)
    static AKZ_HD bool from_sample(const float (&x0)[8], const float (&y0)[8], const float (&x1)[8], const float (&y1)[8], float epsilon,
                                   float (&f)[9]) {
        return fundamental_from_8(x0, y0, x1, y1, epsilon, f);
    }
    static AKZ_HD bool inlier(const float (&f)[9], float x0, float y0, float x1, float y1, float eps) {
        return fundamental_error(f, x0, y0, x1, y1) < eps;
    }
};

// The same model for the calls that hand the winner back (akz_remove_outliers_fundamental, akz_match_features_fundamental*):
// f and found are written; without a winner f is the zero model that was evaluated
struct FundamentalRansacModelOut : FundamentalRansac {
    static constexpr bool kModelOut = true;
    static constexpr bool kZeroModelOut = true;
};

// The gate of guided matching for a fundamental matrix (akz_descriptor_match_guided, model_kind 1): the point
// (x1, y1) lies closer than `radius` pixels to the epipolar line F (x0, y0, 1)^T, without a division or a square root, in
// f32 in this order.  Per query (epipolar_line):
//     l_r = (f[3 r] x0 + f[3 r + 1] y0) + f[3 r + 2], r = 0, 1, 2;   n = l0 l0 + l1 l1;   r2n = (radius radius) n
// per train row (epipolar_near): s = (l0 x1 + l1 y1) + l2, passes iff s s < r2n.  Strict: a zero line (F = 0) passes
// nothing, and neither does a NaN anywhere.  F has the convention of fundamental_error (p1^T F p0).
// This is a DISTANCE IN PIXELS and deliberately not the algebraic |p1^T F p0| < epsilon of akz_remove_outliers /
// fundamental_error, whose scale depends on the normalisation of F: a search band wants a width in pixels.
struct EpipolarLine {
    float l0, l1, l2, r2n;
};
AKZ_HD EpipolarLine epipolar_line(const float (&f)[9], float x0, float y0, float radius) {
    EpipolarLine e;
    e.l0 = (f[0] * x0 + f[1] * y0) + f[2];
    e.l1 = (f[3] * x0 + f[4] * y0) + f[5];
    e.l2 = (f[6] * x0 + f[7] * y0) + f[8];
    const float n = e.l0 * e.l0 + e.l1 * e.l1, r2 = radius * radius;
    e.r2n = r2 * n;
    return e;
}
AKZ_HD bool epipolar_near(const EpipolarLine& e, float x1, float y1) {
    const float s = (e.l0 * x1 + e.l1 * y1) + e.l2;
    return s * s < e.r2n;
}
AKZ_HD bool fundamental_near_line(const float (&f)[9], float x0, float y0, float x1, float y1, float radius) {
    return epipolar_near(epipolar_line(f, x0, y0, radius), x1, y1);
}

}  // namespace akz
