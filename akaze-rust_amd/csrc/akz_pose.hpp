// Relative pose from a fundamental matrix and two pinhole cameras -- E, its four (R, t) candidates, the cheirality count of
// every candidate over a match list, the winner, the filtered list and the triangulated points -- as ONE piece of source for the
// host statement (akz_recover_pose_host, akz_pose_api.cpp) and the device kernel (k_pairs_pose, akz_pose.hip), like
// akz_fundamental_refit.hpp for the refit: f64 in a fixed order, no contraction, the same bits on both sides.
// Every sum of three terms below is (t0 + t1) + t2.
//
// Inputs: F (9 x f32, row-major, p1^T F p0 = 0 in pixels) and the cameras of image 0 and image 1, each {fx, fy, cx, cy} (f64):
// K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]], no skew, no distortion.
//
// decompose (pose_decompose):
//   1. E = K1^T F K0.  A = F K0:  A[r][0] = F[r][0] fx0, A[r][1] = F[r][1] fy0, A[r][2] = (F[r][0] cx0 + F[r][1] cy0) + F[r][2];
//      E[0][c] = fx1 A[0][c], E[1][c] = fy1 A[1][c], E[2][c] = (cx1 A[0][c] + cy1 A[1][c]) + A[2][c].
//   2. the Hestenes rotations of akz_fmatrix.hpp on the three rows of a copy of E (a 3 x 9 matrix whose columns 3 .. 8 are zero:
//      jacobi_sweeps_rows<3>).  The rotated rows are sigma_i v_i^T; their norms sqrt((m0 m0 + m1 m1) + m2 m2) are the singular
//      values.  i1 = the row of the largest norm (the first among equals), i2 = the largest of the two others (the first among
//      equals), i3 = the one left: sigma1 >= sigma2 >= sigma3.
//   3. no pose if sigma1 is zero or not finite (sigma[] stays zero).  Else sigma[] = {1, sigma2 / sigma1, sigma3 / sigma1} as f32, and no pose
//      if !(sigma2 > AKZ_FUNDAMENTAL_REFIT_EPSILON sigma1): a zero model, a rank-1 F, a pure rotation in exact data.  sigma3 is ignored.
//   4. v1 = row i1 / sigma1, v2 = row i2 / sigma2; u1 = (E v1) / sigma1, u2 = (E v2) / sigma2 (each component the three-term sum, then
//      the division); u3 = u1 x u2, v3 = v1 x v2 with (a x b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).  U = [u1 u2 u3] and
//      V = [v1 v2 v3] are proper.
//   5. With W = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]:  Ra = U W V^T, Ra[r][c] = (u2[r] v1[c] - u1[r] v2[c]) + u3[r] v3[c];
//      Rb = U W^T V^T, Rb[r][c] = (u1[r] v2[c] - u2[r] v1[c]) + u3[r] v3[c];  t = u3 / |u3|, |u3| = sqrt((u3_0^2 + u3_1^2) + u3_2^2);
//      a |u3| that is zero or not finite: no pose.
//   Candidates, x1 = R x0 + t:  0 = (Ra, +t), 1 = (Ra, -t), 2 = (Rb, +t), 3 = (Rb, -t).
//
// cheirality of one match (x0, y0) <-> (x1, y1) under (R, t) (pose_depths), without a division by the determinant:
//   a = ((x0 - cx0) / fx0, (y0 - cy0) / fy0, 1), b = ((x1 - cx1) / fx1, (y1 - cy1) / fy1, 1) in f64;
//   c = R a, c[r] = (R[r][0] a0 + R[r][1] a1) + R[r][2];
//   cc = c.c, bb = b.b, cb = c.b, bt = b.t, ct = c.t (three-term sums);
//   det = cc bb - cb cb,  n0 = cb bt - ct bb,  n1 = cc bt - cb ct.
//   In front iff det > 0 and n0 > 0 and n1 > 0: the signs of the depths lambda0 = n0 / det, lambda1 = n1 / det at which the rays meet
//   in the least-squares sense.  A NaN passes nothing.  (-t negates bt, ct, n0 and n1 exactly, so pose_front evaluates each R once
//   with +t: candidate -t is in front iff det > 0 and n0 < 0 and n1 < 0.)
//
// winner: in_front[k] = the matches in front under candidate k; the candidate of the largest count, the first among equals; a
// largest count of 0: no pose.  Result (pose_result): r = the winner's R and t = its +-t rounded to f32, winner, found = 1; no
// pose: r, t, winner zero and found 0, sigma and in_front as far as they were computed.
//
// list: with a pose, the matches in front under the winner, in input order; without one, the input unchanged.
//
// structure (pose_point), for a kept match under the winner (R, ts = +-t): lambda0 = n0 / det, lambda1 = n1 / det from pose_depths
// with ts; d = lambda1 b - ts; w[k] = (R[0][k] d0 + R[1][k] d1) + R[2][k] d2 (= R^T d); X[k] = 0.5 (lambda0 a[k] + w[k]), rounded to
// f32: the midpoint of the two rays' closest points in camera 0's frame, at the scale |t| = 1.
#pragma once
#include <cstdint>

#include "../../include/akaze_hip.h"
#include "akz_homography_refit.hpp"

namespace akz {

struct Mat3x9 {
    double v[3][9];
    AKZ_HD double& at(int p, int k) { return v[p][k]; }
};

// the two rotations and the translation of the four candidates
struct PoseCandidates {
    double ra[9], rb[9], t[3];
};

AKZ_HD bool pose_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

AKZ_HD double pose_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// steps 1 .. 5; m: the caller's 3 x 9 matrix (an array on the host, LDS on the device).  sigma: zeros or step 3's.  false: no pose
template <class M>
AKZ_HD bool pose_decompose(M& m, const float* f, const akz_camera& k0, const akz_camera& k1, PoseCandidates& pc, float (&sigma)[3]) {
    sigma[0] = sigma[1] = sigma[2] = 0.0f;
    double a[9], e[9];
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        const double f0 = (double)f[3 * r], f1 = (double)f[3 * r + 1], f2 = (double)f[3 * r + 2];
        a[3 * r + 0] = f0 * k0.fx;
        a[3 * r + 1] = f1 * k0.fy;
        a[3 * r + 2] = (f0 * k0.cx + f1 * k0.cy) + f2;
    }
    AKZ_UNROLL
    for (int c = 0; c < 3; ++c) {
        e[c] = k1.fx * a[c];
        e[3 + c] = k1.fy * a[3 + c];
        e[6 + c] = (k1.cx * a[c] + k1.cy * a[3 + c]) + a[6 + c];
    }
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        AKZ_UNROLL
        for (int k = 0; k < 9; ++k) m.at(r, k) = k < 3 ? e[3 * r + k] : 0.0;
    }
    jacobi_sweeps_rows<3>(m);
    double nrm[3];
    AKZ_UNROLL
    for (int i = 0; i < 3; ++i) nrm[i] = sqrt((m.at(i, 0) * m.at(i, 0) + m.at(i, 1) * m.at(i, 1)) + m.at(i, 2) * m.at(i, 2));
    int i1 = 0;
    if (nrm[1] > nrm[i1]) i1 = 1;
    if (nrm[2] > nrm[i1]) i1 = 2;
    const int ja = i1 == 0 ? 1 : 0, jb = i1 == 2 ? 1 : 2;  // the two others, ascending
    const int i2 = nrm[jb] > nrm[ja] ? jb : ja, i3 = i2 == ja ? jb : ja;
    const double s1 = nrm[i1], s2 = nrm[i2], s3 = nrm[i3];
    if (!(s1 > 0.0) || !pose_finite(s1)) return false;
    sigma[0] = 1.0f;
    sigma[1] = (float)(s2 / s1);
    sigma[2] = (float)(s3 / s1);
    if (!(s2 > (double)AKZ_FUNDAMENTAL_REFIT_EPSILON * s1)) return false;
    double v1[3], v2[3], u1[3], u2[3], u3[3], v3[3];
    AKZ_UNROLL
    for (int k = 0; k < 3; ++k) {
        v1[k] = m.at(i1, k) / s1;
        v2[k] = m.at(i2, k) / s2;
    }
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        u1[r] = pose_dot3(e + 3 * r, v1) / s1;
        u2[r] = pose_dot3(e + 3 * r, v2) / s2;
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
    v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
    v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
    AKZ_UNROLL
    for (int r = 0; r < 3; ++r) {
        AKZ_UNROLL
        for (int c = 0; c < 3; ++c) {
            pc.ra[3 * r + c] = (u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c];
            pc.rb[3 * r + c] = (u1[r] * v2[c] - u2[r] * v1[c]) + u3[r] * v3[c];
        }
    }
    const double n3 = sqrt(pose_dot3(u3, u3));
    if (!(n3 > 0.0) || !pose_finite(n3)) return false;
    AKZ_UNROLL
    for (int k = 0; k < 3; ++k) pc.t[k] = u3[k] / n3;
    return true;
}

// the normalised rays of one match
AKZ_HD void pose_rays(float x0, float y0, float x1, float y1, const akz_camera& k0, const akz_camera& k1, double (&a)[3], double (&b)[3]) {
    a[0] = ((double)x0 - k0.cx) / k0.fx;
    a[1] = ((double)y0 - k0.cy) / k0.fy;
    a[2] = 1.0;
    b[0] = ((double)x1 - k1.cx) / k1.fx;
    b[1] = ((double)y1 - k1.cy) / k1.fy;
    b[2] = 1.0;
}

AKZ_HD void pose_depths(const double* r, const double* t, const double (&a)[3], const double (&b)[3], double& det, double& n0, double& n1) {
    double c[3];
    AKZ_UNROLL
    for (int k = 0; k < 3; ++k) c[k] = (r[3 * k] * a[0] + r[3 * k + 1] * a[1]) + r[3 * k + 2];
    const double cc = pose_dot3(c, c), bb = pose_dot3(b, b), cb = pose_dot3(c, b), bt = pose_dot3(b, t), ct = pose_dot3(c, t);
    det = cc * bb - cb * cb;
    n0 = cb * bt - ct * bb;
    n1 = cc * bt - cb * ct;
}

// bit k: the match is in front under candidate k
AKZ_HD unsigned pose_front(const PoseCandidates& pc, const double (&a)[3], const double (&b)[3]) {
    double det, n0, n1;
    unsigned bits = 0;
    pose_depths(pc.ra, pc.t, a, b, det, n0, n1);
    if (det > 0.0 && n0 > 0.0 && n1 > 0.0) bits |= 1u;
    if (det > 0.0 && n0 < 0.0 && n1 < 0.0) bits |= 2u;
    pose_depths(pc.rb, pc.t, a, b, det, n0, n1);
    if (det > 0.0 && n0 > 0.0 && n1 > 0.0) bits |= 4u;
    if (det > 0.0 && n0 < 0.0 && n1 < 0.0) bits |= 8u;
    return bits;
}

// the candidate of the largest count, the first among equals; false: the largest count is 0
AKZ_HD bool pose_winner(const uint32_t (&in_front)[4], uint32_t& winner) {
    uint32_t w = 0;
    AKZ_UNROLL
    for (uint32_t k = 1; k < 4; ++k)
        if (in_front[k] > in_front[w]) w = k;
    winner = w;
    return in_front[w] > 0;
}

// the winner's rotation and signed translation
AKZ_HD void pose_of_candidate(const PoseCandidates& pc, uint32_t winner, double (&r)[9], double (&ts)[3]) {
    AKZ_UNROLL
    for (int k = 0; k < 9; ++k) r[k] = winner < 2 ? pc.ra[k] : pc.rb[k];
    AKZ_UNROLL
    for (int k = 0; k < 3; ++k) ts[k] = (winner & 1u) ? -pc.t[k] : pc.t[k];
}

// the result of a pair; ok: the decomposition gave candidates
AKZ_HD void pose_result(bool ok, const PoseCandidates& pc, const float (&sigma)[3], const uint32_t (&in_front)[4], akz_pose& out) {
    uint32_t winner = 0;
    const bool found = ok && pose_winner(in_front, winner);
    double r[9], ts[3];
    if (found) pose_of_candidate(pc, winner, r, ts);
    AKZ_UNROLL
    for (int k = 0; k < 9; ++k) out.r[k] = found ? (float)r[k] : 0.0f;
    AKZ_UNROLL
    for (int k = 0; k < 3; ++k) {
        out.t[k] = found ? (float)ts[k] : 0.0f;
        out.sigma[k] = sigma[k];
    }
    AKZ_UNROLL
    for (int k = 0; k < 4; ++k) out.in_front[k] = in_front[k];
    out.winner = found ? winner : 0u;
    out.found = found ? 1 : 0;
}

// X of a match under (r, ts)
AKZ_HD void pose_point(const double (&r)[9], const double (&ts)[3], const double (&a)[3], const double (&b)[3], float (&x)[3]) {
    double det, n0, n1;
    pose_depths(r, ts, a, b, det, n0, n1);
    const double l0 = n0 / det, l1 = n1 / det;
    const double d[3] = {l1 * b[0] - ts[0], l1 * b[1] - ts[1], l1 * b[2] - ts[2]};
    AKZ_UNROLL
    for (int k = 0; k < 3; ++k) {
        const double w = (r[k] * d[0] + r[3 + k] * d[1]) + r[6 + k] * d[2];
        x[k] = (float)(0.5 * (l0 * a[k] + w));
    }
}

}  // namespace akz
