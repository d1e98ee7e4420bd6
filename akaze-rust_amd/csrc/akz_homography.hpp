// The model of one homography RANSAC trial -- the 4-point DLT with Hartley normalisation -- as ONE piece of source for the
// host path (akz_ransac.cpp) and the device kernels (akz_ransac_kernels.hip), like akz_fmatrix.hpp for the fundamental
// matrix: f64 arithmetic in a fixed order, no contraction (-ffp-contract=off on both sides), the same bits on both.
// The reference has no homography; this is an addition.
//
//   * normalisation, per image over the 4 sample points (f32 widened to f64): centroid c = (((p0 + p1) + p2) + p3) / 4,
//     mean distance d = (((|p0 - c| + |p1 - c|) + |p2 - c|) + |p3 - c|) / 4, s = sqrt(2) / d, point -> s (p - c);
//     d == 0: no model;
//   * degenerate samples are refused before the decomposition: in either image a triple of the four whose cross product in
//     normalised coordinates has |det| <= 1e-9 (collinear, or two equal points), or a triple whose orientation sign differs
//     between the two images (a plane seen from its front never flips orientation);
//   * design matrix: per correspondence (x, y) -> (u, v), normalised, in sample order, the rows
//     [-x, -y, -1, 0, 0, 0, u x, u y, u] and [0, 0, 0, -x, -y, -1, v x, v y, v];
//   * null vector: the one-sided Jacobi sweeps of akz_fmatrix.hpp; all 8 rotated row norms above epsilon_model (as f32),
//     else no model; the rotated rows r_i are orthogonal and span the row space, so n_k = e_k - sum_i (r_i[k] / |r_i|^2) r_i
//     lies in the null space: the first k with the largest |n_k|, normalised, is H^ (row-major);
//   * H = T1^-1 H^ T0; |H[8]| <= 1e-12 ||H||_F (the origin maps to infinity): no model; else H / H[8], rounded to f32.
#pragma once
#include "akz_fmatrix.hpp"

#if defined(__HIPCC__)
#define AKZ_NOUNROLL _Pragma("unroll 1")  // (loops the device must not unroll: their bodies would hold the matrix in registers)
#else
#define AKZ_NOUNROLL
#endif

namespace akz {

// The sample after normalisation and the degeneracy test: normalised points of both images, and T0, T1 as (c, s)
struct HomSample {
    double x0[4], y0[4], x1[4], y1[4];
    double c0x, c0y, s0, c1x, c1y, s1;
};

AKZ_HD bool hom_normalise(const float (&x)[4], const float (&y)[4], double (&nx)[4], double (&ny)[4], double& cx, double& cy,
                          double& s) {
    cx = ((((double)x[0] + (double)x[1]) + (double)x[2]) + (double)x[3]) * 0.25;
    cy = ((((double)y[0] + (double)y[1]) + (double)y[2]) + (double)y[3]) * 0.25;
    double d = 0.0;
    AKZ_UNROLL
    for (int i = 0; i < 4; ++i) {
        const double dx = (double)x[i] - cx, dy = (double)y[i] - cy;
        d += sqrt(dx * dx + dy * dy);
    }
    d = d * 0.25;
    if (!(d > 0.0)) return false;
    s = 1.4142135623730951 / d;  // sqrt(2) / d
    AKZ_UNROLL
    for (int i = 0; i < 4; ++i) {
        nx[i] = s * ((double)x[i] - cx);
        ny[i] = s * ((double)y[i] - cy);
    }
    return true;
}

// (b - a) x (c - a)
AKZ_HD double hom_cross(const double (&x)[4], const double (&y)[4], int a, int b, int c) {
    return (x[b] - x[a]) * (y[c] - y[a]) - (y[b] - y[a]) * (x[c] - x[a]);
}

// normalisation of both images and the degeneracy rules; false: no model
AKZ_HD bool hom_prepare(const float (&x0)[4], const float (&y0)[4], const float (&x1)[4], const float (&y1)[4], HomSample& hs) {
    if (!hom_normalise(x0, y0, hs.x0, hs.y0, hs.c0x, hs.c0y, hs.s0)) return false;
    if (!hom_normalise(x1, y1, hs.x1, hs.y1, hs.c1x, hs.c1y, hs.s1)) return false;
    const int tri[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
    bool ok = true;
    AKZ_UNROLL
    for (int t = 0; t < 4; ++t) {
        const double d0 = hom_cross(hs.x0, hs.y0, tri[t][0], tri[t][1], tri[t][2]);
        const double d1 = hom_cross(hs.x1, hs.y1, tri[t][0], tri[t][1], tri[t][2]);
        if (!(fabs(d0) > 1e-9) || !(fabs(d1) > 1e-9) || ((d0 > 0.0) != (d1 > 0.0))) ok = false;
    }
    return ok;
}

// rows 2 i and 2 i + 1 of the design matrix (correspondence i of the sample); i must be a constant after unrolling on the
// device (the sample lives in registers)
template <class M>
AKZ_HD void hom_rows(M& m, int i, double x, double y, double u, double v) {
    const double r0[9] = {-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u};
    const double r1[9] = {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v};
    AKZ_UNROLL
    for (int k = 0; k < 9; ++k) {
        m.at(2 * i, k) = r0[k];
        m.at(2 * i + 1, k) = r1[k];
    }
}

// the model from 8 orthogonal rows (rows 0..7 of m, all of norm > 0) and the normalisation (c0, s0, c1, s1): the null-vector
// projection, the denormalisation, the H[8] rule and the rounding to f32; false: H[8] ~ 0.  Shared by the trial model below
// and by the refit on the inliers (akz_homography_refit.hpp).
template <class M>
AKZ_HD bool hom_model_from_rows(M& m, double c0x, double c0y, double s0, double c1x, double c1y, double s1, float (&h)[9]) {
    // (row by row, the row reloaded per k: the device keeps one row in registers instead of the whole matrix)
    double best[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, best_n = -1.0;
    AKZ_NOUNROLL
    for (int k = 0; k < 9; ++k) {
        double n[9];
        AKZ_UNROLL
        for (int j = 0; j < 9; ++j) n[j] = j == k ? 1.0 : 0.0;
        AKZ_NOUNROLL
        for (int i = 0; i < 8; ++i) {
            double r[9], nr = 0.0;
            AKZ_UNROLL
            for (int j = 0; j < 9; ++j) {
                r[j] = m.at(i, j);
                nr += r[j] * r[j];
            }
            const double c = m.at(i, k) * (1.0 / nr);  // (full rank: nr > 0)
            AKZ_UNROLL
            for (int j = 0; j < 9; ++j) n[j] = n[j] - c * r[j];
        }
        double nn = 0.0;
        AKZ_UNROLL
        for (int j = 0; j < 9; ++j) nn += n[j] * n[j];
        if (nn > best_n) {  // the first k among equals
            best_n = nn;
            AKZ_UNROLL
            for (int j = 0; j < 9; ++j) best[j] = n[j];
        }
    }
    if (!(best_n > 0.0)) return false;
    const double bn = sqrt(best_n);
    double hn[9];
    AKZ_UNROLL
    for (int j = 0; j < 9; ++j) hn[j] = best[j] / bn;
    // A = H^ T0 with T0 = [[s0, 0, -s0 c0x], [0, s0, -s0 c0y], [0, 0, 1]]
    const double tx0 = -(s0 * c0x), ty0 = -(s0 * c0y);
    double a[9];
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        a[3 * r + 0] = hn[3 * r + 0] * s0;
        a[3 * r + 1] = hn[3 * r + 1] * s0;
        a[3 * r + 2] = (hn[3 * r + 0] * tx0 + hn[3 * r + 1] * ty0) + hn[3 * r + 2];
    }
    // H = T1^-1 A with T1^-1 = [[1 / s1, 0, c1x], [0, 1 / s1, c1y], [0, 0, 1]]
    const double is1 = 1.0 / s1;
    double H[9];
    AKZ_UNROLL
    for (int col = 0; col < 3; ++col) {
        H[col] = a[col] * is1 + c1x * a[6 + col];
        H[3 + col] = a[3 + col] * is1 + c1y * a[6 + col];
        H[6 + col] = a[6 + col];
    }
    double fro = 0.0;
    AKZ_UNROLL
    for (int j = 0; j < 9; ++j) fro += H[j] * H[j];
    fro = sqrt(fro);
    if (!(fabs(H[8]) > 1e-12 * fro)) return false;
    AKZ_UNROLL
    for (int j = 0; j < 9; ++j) h[j] = (float)(H[j] / H[8]);
    return true;
}

// the model from the rotated matrix and the normalisation (c0, s0, c1, s1); false: rank < 8 at `epsilon` or H[8] ~ 0
template <class M>
AKZ_HD bool hom_model_from_rotated(M& m, float epsilon, double c0x, double c0y, double s0, double c1x, double c1y, double s1,
                                   float (&h)[9]) {
    bool full = false;
    (void)smallest_singular(m, epsilon, &full);
    if (!full) return false;
    return hom_model_from_rows(m, c0x, c0y, s0, c1x, c1y, s1, h);
}

// x0, y0 from keypoints_0 and x1, y1 from keypoints_1 of the four sampled matches -> H (row-major, H[8] = 1)
AKZ_HD bool homography_from_4(const float (&x0)[4], const float (&y0)[4], const float (&x1)[4], const float (&y1)[4], float epsilon,
                              float (&h)[9]) {
    HomSample hs;
    if (!hom_prepare(x0, y0, x1, y1, hs)) return false;
    Mat8x9 m;
    for (int i = 0; i < 4; ++i) hom_rows(m, i, hs.x0[i], hs.y0[i], hs.x1[i], hs.y1[i]);
    jacobi_sweeps(m);
    return hom_model_from_rotated(m, epsilon, hs.c0x, hs.c0y, hs.s0, hs.c1x, hs.c1y, hs.s1, h);
}

// The one-way transfer error |H p0 - p1| < eps without a division, in f32 in this order:
// w = (h6 x0 + h7 y0) + h8, U = (h0 x0 + h1 y0) + h2, V = (h3 x0 + h4 y0) + h5, du = U - x1 w, dv = V - y1 w,
// inlier iff w > 0 and du du + dv dv < (eps w) (eps w)
AKZ_HD bool homography_inlier(const float (&h)[9], float x0, float y0, float x1, float y1, float eps) {
    const float w = (h[6] * x0 + h[7] * y0) + h[8];
    const float U = (h[0] * x0 + h[1] * y0) + h[2];
    const float V = (h[3] * x0 + h[4] * y0) + h[5];
    const float du = U - x1 * w, dv = V - y1 * w, ew = eps * w;
    return w > 0.0f && du * du + dv * dv < ew * ew;
}
// The homography as a RANSAC model (see FundamentalRansac)
struct HomographyRansac {
    static constexpr int K = 4;
    static constexpr bool kKeepAllWithoutWinner = true;  // no trial with an inlier: every match is kept whatever epsilon is
    static constexpr bool kModelOut = true;              // H and found are handed back (found = 0: H zeros on the device)
    static constexpr bool kZeroModelOut = false;         // (the host leaves h alone where there is no winner)
    static AKZ_HD bool from_sample(const float (&x0)[4], const float (&y0)[4], const float (&x1)[4], const float (&y1)[4], float epsilon,
                                   float (&h)[9]) {
        return homography_from_4(x0, y0, x1, y1, epsilon, h);
    }
    static AKZ_HD bool inlier(const float (&h)[9], float x0, float y0, float x1, float y1, float eps) {
        return homography_inlier(h, x0, y0, x1, y1, eps);
    }
};
// homography_inlier in two halves for a scan that tests one (x0, y0) against many (x1, y1) (akz_guided.hip): what depends
// on the query alone is formed once -- the same operations on the same values, so transfer_near(transfer_disc(h, x0, y0,
// eps), x1, y1) has the bits of homography_inlier(h, x0, y0, x1, y1, eps).
struct TransferDisc {
    float U, V, w, ew2;
};
AKZ_HD TransferDisc transfer_disc(const float (&h)[9], float x0, float y0, float eps) {
    TransferDisc t;
    t.w = (h[6] * x0 + h[7] * y0) + h[8];
    t.U = (h[0] * x0 + h[1] * y0) + h[2];
    t.V = (h[3] * x0 + h[4] * y0) + h[5];
    const float ew = eps * t.w;
    t.ew2 = ew * ew;
    return t;
}
AKZ_HD bool transfer_near(const TransferDisc& t, float x1, float y1) {
    const float du = t.U - x1 * t.w, dv = t.V - y1 * t.w;
    return t.w > 0.0f && du * du + dv * dv < t.ew2;
}

}  // namespace akz
