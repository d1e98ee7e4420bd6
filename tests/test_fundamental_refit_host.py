"""The RANSAC fundamental matrix handed back and refitted on its inliers, on the host (akz_remove_outliers_fundamental,
akz_refine_fundamental_matrix; no GPU call): declarations and refusals, the model and the list against akz_remove_outliers and
the inlier rule restated in numpy f32, the fit against an independent numpy statement (Hartley normalisation, np.linalg.svd of
the N-row design matrix, the smallest singular value of F^ zeroed), the loop's promises, the cases without a model, and the
gain in accuracy on two-view scenes against the unrefined winner of the same draws."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_homography_host import _ident_matches, _kp
from test_match_pairs_host import ROOT, _color, _status

EPS_MODEL = 0.05  # the reference's epsilon_model of the trial model
NEW_SYMBOLS = ("akz_remove_outliers_fundamental", "akz_refine_fundamental_matrix", "akz_match_features_fundamental",
               "akz_match_features_fundamental_pairs", "akz_match_features_fundamental_refined",
               "akz_match_features_fundamental_refined_pairs", "akz_match_features_fundamental_guided",
               "akz_match_features_fundamental_guided_pairs", "akz_match_features_fundamental_refined_guided",
               "akz_match_features_fundamental_refined_guided_pairs")


# ---- two-view scenes ---------------------------------------------------------------------------------------------------------
def _rotation(rv):
    th = np.linalg.norm(rv)
    if th == 0.0:
        return np.eye(3)
    k = rv / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx


def two_view_scene(seed, n, sigma=0.7, outliers=0.2):
    """A camera of f = 1200 px at 1920 x 1080 (principal point at the centre) sees n points uniform in [-4, 4] x [-2.5, 2.5] x
    [4, 12] from two poses: rotation vector uniform in +-0.15 rad per axis, t = (+-U(0.5, 1), U(-0.3, 0.3), U(-0.5, 0.5)).
    Image 1 gets N(0, sigma) px of noise, a share `outliers` of its points is displaced by 50 .. 400 px.  Returns (p0, p1 true,
    p1 observed, outlier mask, F_true of unit norm with p1^T F p0 = 0), coordinates in f64."""
    rng = np.random.default_rng(seed)
    k = np.array([[1200.0, 0, 960.0], [0, 1200.0, 540.0], [0, 0, 1]])
    x = np.c_[rng.uniform(-4, 4, n), rng.uniform(-2.5, 2.5, n), rng.uniform(4, 12, n)]
    r = _rotation(rng.uniform(-0.15, 0.15, 3))
    t = np.array([rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1), rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5)])
    p0 = x @ k.T
    p0 = p0[:, :2] / p0[:, 2:]
    p1 = (x @ r.T + t) @ k.T
    p1 = p1[:, :2] / p1[:, 2:]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    ki = np.linalg.inv(k)
    f = ki.T @ tx @ r @ ki
    f /= np.linalg.norm(f)
    out = rng.uniform(size=n) < outliers
    q1 = p1 + rng.normal(0, sigma, (n, 2))
    ang, dist = rng.uniform(0, 2 * np.pi, n), rng.uniform(50, 400, n)
    q1[out] += (np.c_[np.cos(ang), np.sin(ang)] * dist[:, None])[out]
    return p0, p1, q1, out, f


def scene_epsilon(f_true, p0):
    """2 px in the algebraic units of |p1^T F p0| at unit norm: 2 x the median over the matches of sqrt(l0^2 + l1^2), l = F p0"""
    line = np.c_[p0, np.ones(len(p0))] @ f_true.T
    return float(2.0 * np.median(np.sqrt(line[:, 0] ** 2 + line[:, 1] ** 2)))


def epipolar_error(f, p0, p1):
    """mean symmetric epipolar distance (px) of the correspondences p0 <-> p1 under f (p1^T f p0 = 0)"""
    f = np.asarray(f, np.float64).reshape(3, 3)
    a, b = np.c_[p0, np.ones(len(p0))], np.c_[p1, np.ones(len(p1))]
    l1, l0 = a @ f.T, b @ f
    s = np.abs((b * l1).sum(axis=1))
    return float(0.5 * (s / np.sqrt(l1[:, 0] ** 2 + l1[:, 1] ** 2) + s / np.sqrt(l0[:, 0] ** 2 + l0[:, 1] ** 2)).mean())


def error_rule(f, k0, k1, matches, eps):
    """fundamental_error(f, ..) < eps of the RANSAC in numpy float32, in its expression order"""
    f = np.asarray(f, np.float32).reshape(9)
    x0, y0 = k0["x"][matches["index_0"]].astype(np.float32), k0["y"][matches["index_0"]].astype(np.float32)
    x1, y1 = k1["x"][matches["index_1"]].astype(np.float32), k1["y"][matches["index_1"]].astype(np.float32)
    r0, r1, r2 = (x1 * f[0] + y1 * f[3]) + f[6], (x1 * f[1] + y1 * f[4]) + f[7], (x1 * f[2] + y1 * f[5]) + f[8]
    return np.abs((r0 * x0 + r1 * y0) + r2) < np.float32(eps)


def scene_case(amd, seed, n, **kw):
    """-> (k0, k1, matches in list order, scene)"""
    sc = two_view_scene(seed, n, **kw)
    return _kp(amd, sc[0].astype(np.float32)), _kp(amd, sc[2].astype(np.float32)), _ident_matches(amd, n), sc


def _bits(f):
    return np.asarray(f, np.float32).reshape(9).view(np.uint32)


# ---- declarations and refusals ---------------------------------------------------------------------------------------------
def test_symbols_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert L.akz_abi_version() == 6
    assert re.search(r"#define\s+AKZ_FUNDAMENTAL_REFIT_EPSILON\s+1e-6f", hdr)
    for name in NEW_SYMBOLS:
        assert callable(getattr(amd, name[4:])), name
    for name in NEW_SYMBOLS[3::2]:
        assert callable(getattr(amd.Context, name[4:])), name


def test_refusals(amd):
    L, bad = amd.lib(), _status(amd)
    k0, k1, m, sc = scene_case(amd, 5, 20, outliers=0.0)
    out = np.zeros(20, amd.MATCH_DTYPE)
    n = C.c_uint64(12345)
    fout = np.full(9, 7.0, np.float32)
    it = C.c_uint32(99)
    fin = np.ascontiguousarray(sc[4].astype(np.float32).reshape(9))
    fp = C.POINTER(C.c_float)

    def call(k0p=k0.ctypes.data, n0=len(k0), k1p=k1.ctypes.data, n1=len(k1), mp=m.ctypes.data, nm=len(m),
             fin_p=fin.ctypes.data_as(fp), eps=3.0, outp=out.ctypes.data, np_=C.byref(n)):
        return L.akz_refine_fundamental_matrix(k0p, n0, k1p, n1, mp, nm, fin_p, eps, 8, outp, np_, fout.ctypes.data_as(fp), C.byref(it))
    assert call(np_=None) == bad
    assert call(mp=None) == bad
    assert call(outp=None) == bad
    assert call(fin_p=None) == bad
    for eps in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert call(eps=eps) == bad, eps
    assert call(n0=19) == bad and call(n1=19) == bad      # an index past a keypoint array
    assert call(k0p=None) == bad and call(k1p=None) == bad
    # nothing was written by a refused call
    assert n.value == 12345 and it.value == 99 and np.all(fout == 7.0) and not out.view(np.uint8).any()
    # NULL f_out and iterations are allowed; an empty list is AKZ_OK
    assert L.akz_refine_fundamental_matrix(k0.ctypes.data, len(k0), k1.ctypes.data, len(k1), m.ctypes.data, len(m), fin.ctypes.data_as(fp),
                                           3.0, 8, out.ctypes.data, C.byref(n), None, None) == 0
    assert n.value <= 20
    assert L.akz_refine_fundamental_matrix(None, 0, None, 0, None, 0, fin.ctypes.data_as(fp), 3.0, 8, None, C.byref(n), None, None) == 0
    assert n.value == 0
    # akz_remove_outliers_fundamental: the refusals of akz_remove_outliers, before a draw; NULL f and found are allowed
    amd.random_seed(42, 69)
    fresh = _color(amd)
    amd.random_seed(42, 69)
    found = C.c_int(5)
    n.value = 12345
    args = (k0.ctypes.data, len(k0), k1.ctypes.data, len(k1), m.ctypes.data, len(m), 10, EPS_MODEL, 3.0)
    assert L.akz_remove_outliers_fundamental(*args, out.ctypes.data, None, fout.ctypes.data_as(fp), C.byref(found)) == bad
    assert L.akz_remove_outliers_fundamental(*args[:1], 19, *args[2:], out.ctypes.data, C.byref(n), fout.ctypes.data_as(fp),
                                             C.byref(found)) == bad
    assert n.value == 12345 and found.value == 5 and np.all(fout == 7.0)
    assert _color(amd) == fresh
    amd.random_seed(42, 69)
    assert L.akz_remove_outliers_fundamental(*args, out.ctypes.data, C.byref(n), None, None) == 0
    amd.random_seed(42, 69)
    assert np.array_equal(out[:n.value], amd.remove_outliers(k0, k1, m, 10, EPS_MODEL, 3.0))


# ---- the model handed back -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,trials", [(8, 50), (9, 50), (65, 200), (257, 500), (1000, 500), (257, 0), (257, 1)])
def test_remove_outliers_fundamental_is_remove_outliers_with_the_model(amd, n, trials):
    k0, k1, m, sc = scene_case(amd, 300 + n, n)
    m["distance"] = np.arange(n) % 97
    eps = scene_epsilon(sc[4], sc[0])
    amd.random_seed(42, 69)
    exp = amd.remove_outliers(k0, k1, m, trials, EPS_MODEL, eps)
    after_exp = _color(amd)
    amd.random_seed(42, 69)
    kept, f = amd.remove_outliers_fundamental(k0, k1, m, trials, EPS_MODEL, eps)
    assert _color(amd) == after_exp                       # the same draws
    assert kept.dtype == exp.dtype and np.array_equal(kept, exp), (len(kept), len(exp))
    if trials == 0:
        assert f is None and np.array_equal(kept, m)      # the zero model is evaluated: error 0 everywhere
    if f is not None:
        assert f.dtype == np.float32 and f.shape == (3, 3)
        assert abs(float(np.linalg.norm(f.astype(np.float64))) - 1.0) < 1e-6
        assert np.array_equal(kept, m[error_rule(f, k0, k1, m, eps)])
        assert len(kept) > 0
    else:
        assert np.array_equal(kept, m[error_rule(np.zeros(9), k0, k1, m, eps)])
    if trials >= 200:
        assert f is not None, (n, trials)


def test_fewer_than_eight_matches(amd):
    k0, k1, m, sc = scene_case(amd, 11, 20)
    fp = C.POINTER(C.c_float)
    for n in range(8):
        amd.random_seed(42, 69)
        fresh = _color(amd)
        amd.random_seed(42, 69)
        kept, f = amd.remove_outliers_fundamental(k0, k1, m[:n], 100, EPS_MODEL, 1e-3)
        assert f is None and np.array_equal(kept, m[:n])
        assert _color(amd) == fresh                       # nothing was drawn
    # the C call: found 0, f zeros
    fout, found, cnt = np.full(9, 7.0, np.float32), C.c_int(5), C.c_uint64()
    out = np.zeros(20, amd.MATCH_DTYPE)
    assert amd.lib().akz_remove_outliers_fundamental(k0.ctypes.data, len(k0), k1.ctypes.data, len(k1), m.ctypes.data, 7, 100, EPS_MODEL,
                                                     1e-3, out.ctypes.data, C.byref(cnt), fout.ctypes.data_as(fp), C.byref(found)) == 0
    assert cnt.value == 7 and found.value == 0 and not fout.any()


# ---- the fit against numpy -------------------------------------------------------------------------------------------------
def _hartley(p):
    c = p.mean(axis=0)
    s = np.sqrt(2.0) / np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    return s * (p - c), np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])


def numpy_fundamental_n(p0, p1):
    """The normalised N-point algorithm with numpy alone: Hartley normalisation, the N x 9 design matrix (entry 3 i + j is
    p_i q_j), its null vector from np.linalg.svd, the smallest singular value of F^ zeroed, F = T1^T F' T0 at unit norm."""
    a0, t0 = _hartley(np.asarray(p0, np.float64))
    a1, t1 = _hartley(np.asarray(p1, np.float64))
    p, q = np.c_[a0, np.ones(len(a0))], np.c_[a1, np.ones(len(a1))]
    a = (p[:, :, None] * q[:, None, :]).reshape(len(p), 9)
    fh = np.linalg.svd(a)[2][-1].reshape(3, 3).T
    u, s, vt = np.linalg.svd(fh)
    s[2] = 0.0
    f = t1.T @ (u * s) @ vt @ t0
    return f / np.linalg.norm(f)


def test_fit_equals_numpy(amd):
    """One fit over a list that is all inliers equals the numpy statement after sign alignment within a relative Frobenius
    difference of 3e-7, and is of rank 2 (sigma_3 <= 1e-6 sigma_1 in f64).  The worst difference seen over these 72 sets is
    2.95e-8 -- the rounding of the result to f32, 2^-24 = 6e-8 per entry at most, and nothing else -- and the bound is ten
    times that."""
    worst = 0.0
    for n in (8, 9, 255, 256, 257, 3001):
        for sigma in (0.0, 0.7):
            for seed in range(6):
                sc = two_view_scene(1000 * n + seed + int(sigma * 10), n, sigma=sigma, outliers=0.0)
                a, b = sc[0].astype(np.float32), sc[2].astype(np.float32)
                exp = numpy_fundamental_n(a, b)
                m = _ident_matches(amd, n)
                kept, got, its = amd.refine_fundamental_matrix(_kp(amd, a), _kp(amd, b), m, sc[4], 1e9, 1)
                assert its == 1 and np.array_equal(kept, m), (n, sigma, seed, its)
                assert got.dtype == np.float32
                g = got.astype(np.float64)
                if (g * exp).sum() < 0:
                    g = -g
                rel = float(np.linalg.norm(g - exp) / np.linalg.norm(exp))
                sv = np.linalg.svd(got.astype(np.float64), compute_uv=False)
                worst = max(worst, rel)
                print(n, sigma, seed, "rel", rel, "sigma3 / sigma1", sv[2] / sv[0])
                assert rel <= 3e-7, (n, sigma, seed, rel)
                assert sv[2] <= 1e-6 * sv[0], (n, sigma, seed, sv)
                assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1.0) < 1e-6
    print("worst", worst)


# ---- the loop --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def winners(amd):
    """the quality scenes with the winner of 500 trials (computed once, left unchanged):
    (k0, k1, matches, scene, eps, kept, F winner) per (seed, n)"""
    cases = []
    for seed, n in QUALITY_SCENES:
        k0, k1, m, sc = scene_case(amd, seed, n)
        eps = scene_epsilon(sc[4], sc[0])
        amd.random_seed(42, 69)
        kept, f = amd.remove_outliers_fundamental(k0, k1, m, 500, EPS_MODEL, eps)
        cases.append((k0, k1, m, sc, eps, kept, f))
    return cases


@pytest.mark.parametrize("max_it", [0, 1, 2, 8])
def test_loop(amd, winners, max_it):
    for k0, k1, m, _, eps, kept_in, f_in in winners:
        assert f_in is not None
        kept, f, its = amd.refine_fundamental_matrix(k0, k1, m, f_in, eps, max_it)
        assert len(kept) >= len(kept_in), (len(kept), len(kept_in))   # never fewer inliers
        assert its <= max_it
        assert np.array_equal(kept, m[error_rule(f, k0, k1, m, eps)])
        assert np.all(np.isfinite(f))
        if max_it == 0 or its == 0:
            assert np.array_equal(_bits(f), _bits(f_in)) and np.array_equal(kept, kept_in)
    if max_it > 0:
        prev = [amd.refine_fundamental_matrix(k0, k1, m, f_in, eps, max_it - 1) for k0, k1, m, _, eps, _, f_in in winners]
        cur = [amd.refine_fundamental_matrix(k0, k1, m, f_in, eps, max_it) for k0, k1, m, _, eps, _, f_in in winners]
        assert all(len(c[0]) >= len(p[0]) and c[2] >= p[2] for c, p in zip(cur, prev))


def _unchanged(amd, k0, k1, m, f_in, eps, expect_kept):
    for max_it in (1, 8):
        kept, f, its = amd.refine_fundamental_matrix(k0, k1, m, f_in, eps, max_it)
        assert its == 0
        assert np.array_equal(_bits(f), _bits(f_in)) and np.all(np.isfinite(f))
        assert np.array_equal(kept, m[expect_kept])


def test_no_model(amd):
    sc = two_view_scene(3, 12, sigma=0.0, outliers=0.0)
    p0, p1, f_true = sc[0].astype(np.float32), sc[1].astype(np.float32), sc[4].astype(np.float32)
    m = _ident_matches(amd, 12)
    all12 = np.ones(12, bool)
    same = np.repeat(np.array([[640.0, 360.0]], np.float32), 12, axis=0)
    zero = np.zeros((3, 3), np.float32)
    # all points equal in image 0 (its mean distance is 0), then in image 1; every match is an inlier of the zero model
    _unchanged(amd, _kp(amd, same), _kp(amd, p1), m, zero, 1.0, all12)
    _unchanged(amd, _kp(amd, p0), _kp(amd, same), m, zero, 1.0, all12)
    # fewer than 8 inliers: 7 of 12 (the others 300 px off their epipolar lines), 0 of 12, and lists of 0 .. 7 matches
    eps = scene_epsilon(sc[4], sc[0]) * 0.05             # 0.1 px: the exact correspondences pass, the displaced ones do not
    far = p1.copy()
    far[7:] += 300.0
    mask = error_rule(f_true, _kp(amd, p0), _kp(amd, far), m, eps)
    assert mask.sum() == 7 and mask[:7].all()
    _unchanged(amd, _kp(amd, p0), _kp(amd, far), m, f_true, eps, mask)
    _unchanged(amd, _kp(amd, p0), _kp(amd, p1 + 300.0), m, f_true, eps, np.zeros(12, bool))
    for n in range(8):
        _unchanged(amd, _kp(amd, p0), _kp(amd, p1), m[:n], f_true, eps, np.ones(n, bool))
    # eight exact inliers do give a model
    kept, f, its = amd.refine_fundamental_matrix(_kp(amd, p0), _kp(amd, p1), m[:8], f_true, eps, 8)
    assert its >= 1 and len(kept) == 8 and np.all(np.isfinite(f))


# ---- quality -----------------------------------------------------------------------------------------------------------------
# (scene seed, n): scenes of the generator above on which the unrefined winner of 500 trials from random_seed(42, 69) lies
# within 2 px of the truth -- the reference's unnormalised 8-point trial model gives no usable winner on about a third of such
# scenes (the 8th singular value of its raw-pixel design matrix sits around epsilon_model), and a refit of such a winner
# rightly changes nothing.  Picked on the host with remove_outliers_fundamental, seeds 0 .. upward, the first eight that qualify per size.
QUALITY_SCENES = [(19, 257), (30, 257), (36, 257), (44, 257), (55, 257), (61, 257), (62, 257), (68, 257),
                  (30, 1000), (31, 1000), (50, 1000), (54, 1000), (56, 1000), (59, 1000), (75, 1000), (78, 1000)]
QUALITY_MEDIAN_RATIO = 0.243  # median of refined / unrefined error over those scenes, as measured


def test_quality(amd, winners):
    """On every scene of QUALITY_SCENES the F refined with max_iterations = 8 has a mean symmetric epipolar distance to the
    noise-free correspondences no larger than the unrefined winner's of the same draws, and at least as many inliers; the
    median ratio refined / unrefined is 0.243 as measured (profiles/r13_fundamental_refit.json; the single ratios run from 0.038
    to 1.0, and 1.0 is a winner whose refit had fewer inliers and was rejected, on 3 of the 16 scenes), asserted with a margin
    of 2x because seeds differ in how good their winner already is.  69 seeds at n = 257 and 79 at n = 1000 were tried for
    these 8 + 8: on this generator the unnormalised trial model gives a usable winner on about one scene in nine."""
    assert len(QUALITY_SCENES) >= 12
    ratios = []
    for (seed, n), (k0, k1, m, sc, eps, kept_in, f_in) in zip(QUALITY_SCENES, winners):
        assert f_in is not None
        before = epipolar_error(f_in, sc[0], sc[1])
        assert before < 2.0, (seed, n, before)            # the precondition the scenes were picked by
        kept, f, its = amd.refine_fundamental_matrix(k0, k1, m, f_in, eps, 8)
        after = epipolar_error(f, sc[0], sc[1])
        print("seed", seed, "n", n, "winner", before, "px", len(kept_in), "inliers; refined", after, "px", len(kept), "inliers;",
              "fits", its, "true inliers", int((~sc[3]).sum()))
        assert after <= before, (seed, n, before, after)
        assert len(kept) >= len(kept_in), (seed, n)
        ratios.append(after / before)
    med = float(np.median(ratios))
    print("median ratio", med)
    assert med <= 2.0 * QUALITY_MEDIAN_RATIO, med
