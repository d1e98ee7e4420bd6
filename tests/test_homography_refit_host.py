"""The refit of the RANSAC homography on its inliers, on the host (akz_refine_homography, no GPU call): the fit against an
independent numpy statement (np.linalg.svd of the N-row normalised design matrix), the loop's promises on noisy
correspondences, the gain in accuracy, exact data, the cases without a model, the documented summation order against a
restatement of the whole statement in plain Python floats (bit for bit), the refusals and the declarations."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from test_gpu_homography import inlier_rule
from test_homography_host import _apply, _ident_matches, _kp, _normalise, synthetic_case
from test_match_pairs_host import ROOT, _status

EPS_MODEL = np.float32(1e-6)  # AKZ_HOMOGRAPHY_EPSILON_MODEL


def _h_true(rng):
    a, sc = rng.uniform(-np.pi, np.pi), rng.uniform(0.7, 1.4)
    return np.array([[sc * np.cos(a), -sc * np.sin(a), rng.uniform(-300, 300)],
                     [sc * np.sin(a), sc * np.cos(a), rng.uniform(-300, 300)],
                     [rng.uniform(-3e-4, 3e-4), rng.uniform(-3e-4, 3e-4), 1.0]])


def _points(rng, h, n):
    """n points of a 1920 x 1080 frame on which h keeps w > 0.2, as f32 values in f64"""
    p0 = np.zeros((0, 2))
    while len(p0) < n:
        c = rng.uniform([0, 0], [1920, 1080], (n, 2))
        p0 = np.r_[p0, c[c @ h[2, :2] + 1.0 > 0.2]]
    return p0[:n].astype(np.float32).astype(np.float64)


# ---- the fit against numpy -------------------------------------------------------------------------------------------------
def numpy_homography_n(p0, p1):
    """numpy_homography of test_homography_host.py for N rows: Hartley normalisation over all N points, the 2N x 9 design
    matrix, the null vector from np.linalg.svd, denormalised, H[2, 2] = 1.  Returns (H, condition number of the 8 nonzero
    singular values of the normalised design matrix)."""
    q0, c0, s0 = _normalise(np.asarray(p0, np.float64))
    q1, c1, s1 = _normalise(np.asarray(p1, np.float64))
    rows = []
    for (x, y), (u, v) in zip(q0, q1):
        rows.append([-x, -y, -1, 0, 0, 0, u * x, u * y, u])
        rows.append([0, 0, 0, -x, -y, -1, v * x, v * y, v])
    a = np.array(rows)
    if len(a) < 9:
        a = np.r_[a, np.zeros((9 - len(a), 9))]
    _, sv, vt = np.linalg.svd(a)
    hn = vt[-1].reshape(3, 3)
    t0 = np.array([[s0, 0, -s0 * c0[0]], [0, s0, -s0 * c0[1]], [0, 0, 1]])
    t1inv = np.array([[1 / s1, 0, c1[0]], [0, 1 / s1, c1[1]], [0, 0, 1]])
    h = t1inv @ hn @ t0
    return h / h[2, 2], sv[0] / sv[7]


def test_fit_equals_numpy(amd):
    """One fit over a list that is all inliers of h_in equals numpy's least-squares DLT within 1e-4 relative per entry wherever
    the normalised N-row design matrix has a condition number below 1e3: the bound and the argument of
    test_model_equals_numpy, and the condition squared by the normal matrix, 1e6 * 2^-52 ~ 2e-10, is still six orders of
    magnitude below the bound."""
    compared = 0
    for n in (4, 5, 9, 100, 1000):
        for seed in range(8):
            rng = np.random.default_rng(100 * n + seed)
            h = _h_true(rng)
            p0 = _points(rng, h, n)
            p1 = (_apply(h, p0) + rng.normal(0, 0.5, (n, 2))).astype(np.float32)
            k0, k1, m = _kp(amd, p0), _kp(amd, p1), _ident_matches(amd, n)
            exp, cond = numpy_homography_n(p0, p1.astype(np.float64))
            if cond >= 1e3:
                continue
            eps = 10.0  # noise of sigma 0.5: every match is an inlier of h_in and of the fit
            assert np.all(inlier_rule(h, k0, k1, m, eps))
            kept, got, its = amd.refine_homography(k0, k1, m, h, eps, 1)
            assert its == 1 and np.array_equal(kept, m), (n, seed, its, len(kept))
            assert got.dtype == np.float32 and got[2, 2] == 1.0
            rel = np.abs(got.astype(np.float64) - exp) / np.abs(exp)
            print(n, seed, "cond", cond, "max rel", rel.max())
            assert np.all(np.abs(got.astype(np.float64) - exp) <= 1e-4 * np.abs(exp)), (n, seed, got, exp)
            compared += 1
    assert compared >= 20, compared


# ---- the loop on noisy correspondences ------------------------------------------------------------------------------------
def noisy_case(amd, seed, n=600, sigma=0.7, outliers=0.35):
    """600 correspondences at 1920 x 1080: inliers H_true p0 + N(0, 0.7 px), 35 % outliers displaced at least 50 px.
    Returns (k0, k1, matches, H_true)."""
    rng = np.random.default_rng(seed)
    h = _h_true(rng)
    p0 = _points(rng, h, n)
    out = rng.uniform(size=n) < outliers
    p1 = _apply(h, p0) + rng.normal(0, sigma, (n, 2)) * (~out)[:, None]
    ang, dist = rng.uniform(0, 2 * np.pi, n), rng.uniform(50, 400, n)
    p1[out] += (np.c_[np.cos(ang), np.sin(ang)] * dist[:, None])[out]
    m = _ident_matches(amd, n)
    m["distance"] = rng.uniform(0, 100, n)
    return _kp(amd, p0), _kp(amd, p1.astype(np.float32)), m, h


@pytest.fixture(scope="module")
def noisy(amd):
    """the eight cases, each with the winner of 1 000 trials at eps 3.0 and its inliers (computed once, left unchanged)"""
    cases = []
    for seed in range(8):
        k0, k1, m, h_true = noisy_case(amd, seed)
        amd.random_seed(42, 69)
        kept, h_in = amd.remove_outliers_homography(k0, k1, m, 1000, float(EPS_MODEL), 3.0)
        assert h_in is not None
        cases.append((k0, k1, m, h_true, kept, h_in))
    return cases


def _grid_rms(h, h_true):
    """RMS transfer error of h against h_true over a 9 x 9 grid of the 1920 x 1080 frame"""
    g = np.stack(np.meshgrid(np.linspace(0, 1920, 9), np.linspace(0, 1080, 9)), -1).reshape(-1, 2)
    return float(np.sqrt(((_apply(h, g) - _apply(h_true, g)) ** 2).sum(axis=1).mean()))


@pytest.mark.parametrize("max_it", [0, 1, 2, 8])
def test_loop(amd, noisy, max_it):
    for seed, (k0, k1, m, _, kept_in, h_in) in enumerate(noisy):
        kept, h, its = amd.refine_homography(k0, k1, m, h_in, 3.0, max_it)
        assert len(kept) >= len(kept_in), (seed, len(kept), len(kept_in))
        assert its <= max_it
        assert np.array_equal(kept, m[inlier_rule(h, k0, k1, m, 3.0)]), seed
        if max_it == 0:
            assert np.array_equal(h.view(np.uint32), h_in.view(np.uint32)) and np.array_equal(kept, kept_in)


def test_accuracy(amd, noisy):
    """After refinement with max_iterations = 8 the RMS transfer error against the true map over a 9 x 9 grid of the frame is
    at most half of the winner's.  (A numpy model of the loop gave ratios of 6.4 to 18 on this generator: the condition has
    room, and it is not a measurement of the code under test.)"""
    for seed, (k0, k1, m, h_true, _, h_in) in enumerate(noisy):
        _, h, its = amd.refine_homography(k0, k1, m, h_in, 3.0, 8)
        before, after = _grid_rms(h_in, h_true), _grid_rms(h, h_true)
        print("seed", seed, "unrefined", before, "refined", after, "ratio", before / after, "fits", its)
        assert after <= 0.5 * before, (seed, before, after)


@pytest.mark.parametrize("seed", range(6))
def test_exact_data_keeps_the_true_inliers(amd, seed):
    k0, k1, m, inl, _ = synthetic_case(amd, seed)
    amd.random_seed(42, 69)
    kept, h_in = amd.remove_outliers_homography(k0, k1, m, 1000, float(EPS_MODEL), 2.0)
    assert h_in is not None and np.array_equal(kept, m[inl])
    refined, h, its = amd.refine_homography(k0, k1, m, h_in, 2.0, 8)
    assert np.array_equal(refined, m[inl]), (len(refined), int(inl.sum()), its)
    assert np.array_equal(refined, m[inlier_rule(h, k0, k1, m, 2.0)])


# ---- no model ----------------------------------------------------------------------------------------------------------------
def _unchanged(amd, k0, k1, m, h_in, eps, expect_kept):
    for max_it in (1, 8):
        kept, h, its = amd.refine_homography(k0, k1, m, h_in, eps, max_it)
        assert its == 0
        assert np.array_equal(h.view(np.uint32), np.asarray(h_in, np.float32).view(np.uint32))
        assert np.array_equal(kept, m[expect_kept])


def test_no_model(amd):
    ident = np.eye(3, dtype=np.float32)
    far = np.array([[900.0, 40.0], [30.0, 700.0], [1500.0, 900.0]])
    # four collinear inliers (and three matches that are none)
    line = np.array([[100.0, 100.0], [200.0, 200.0], [350.0, 350.0], [400.0, 400.0]])
    p0 = np.r_[line, far]
    p1 = np.r_[line, far + 200.0]
    mask = np.arange(7) < 4
    _unchanged(amd, _kp(amd, p0), _kp(amd, p1), _ident_matches(amd, 7), ident, 2.0, mask)
    # all inliers equal in image 0 (its mean distance is 0), then in image 1
    same = np.repeat(np.array([[640.0, 360.0]]), 6, axis=0)
    spread = same + np.array([[0, 0], [0.5, 0], [0, 0.5], [-0.5, 0], [0, -0.5], [0.3, 0.3]])
    all6 = np.ones(6, bool)
    _unchanged(amd, _kp(amd, same), _kp(amd, spread), _ident_matches(amd, 6), ident, 2.0, all6)
    to_point = np.array([[0, 0, 640.0], [0, 0, 360.0], [0, 0, 1.0]], np.float32)
    _unchanged(amd, _kp(amd, spread * 100.0 - [63360.0, 35640.0]), _kp(amd, same), _ident_matches(amd, 6), to_point, 2.0, all6)
    # fewer than 4 inliers: 3 of 7, 0 of 7, and lists of 0 .. 3 matches
    _unchanged(amd, _kp(amd, p0), _kp(amd, np.r_[line[:3], line[3:] + 300.0, far + 200.0]), _ident_matches(amd, 7), ident, 2.0,
               np.arange(7) < 3)
    _unchanged(amd, _kp(amd, p0), _kp(amd, p0 + 500.0), _ident_matches(amd, 7), ident, 2.0, np.zeros(7, bool))
    for n in range(4):
        _unchanged(amd, _kp(amd, p0), _kp(amd, p1), _ident_matches(amd, 7)[:n], ident, 2.0, np.ones(n, bool))


# ---- the whole statement in plain Python floats (f64, one operation at a time: no contraction) -----------------------------
def _f32(v):
    return float(np.float32(v))


def _py_inlier(h, x0, y0, x1, y1, eps):
    f = np.float32
    w = (h[6] * x0 + h[7] * y0) + h[8]
    u = (h[0] * x0 + h[1] * y0) + h[2]
    v = (h[3] * x0 + h[4] * y0) + h[5]
    du, dv, ew = u - x1 * w, v - y1 * w, f(eps) * w
    return bool(w > 0 and du * du + dv * dv < ew * ew)


def _lane_tree(n, member, term, k):
    """every sum of the statement: element i in lane i mod 256, ascending i from +0.0, then p[l] = p[l] + p[l + s]"""
    p = [[0.0] * 256 for _ in range(k)]
    for i in range(n):
        if member[i]:
            t = term(i)
            for j in range(k):
                p[j][i % 256] = p[j][i % 256] + t[j]
    out = []
    for j in range(k):
        s = 128
        while s > 0:
            for l in range(s):
                p[j][l] = p[j][l] + p[j][l + s]
            s >>= 1
        out.append(p[j][0])
    return out


def _py_jacobi_pair(m, p, q):
    alpha = beta = gamma = 0.0
    for k in range(9):
        x, y = m[p][k], m[q][k]
        alpha += x * x
        beta += y * y
        gamma += x * y
    if abs(gamma) <= 1e-15 * math.sqrt(alpha * beta) or gamma == 0.0:
        return False
    zeta = (beta - alpha) / (2.0 * gamma)
    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
    c = 1.0 / math.sqrt(1.0 + t * t)
    sn = c * t
    for k in range(9):
        x, y = m[p][k], m[q][k]
        m[p][k] = c * x - sn * y
        m[q][k] = sn * x + c * y
    return True


def _py_norm(r):
    s = 0.0
    for v in r:
        s += v * v
    return math.sqrt(s)


def _py_fit(x0, y0, x1, y1, member):
    n = len(x0)
    count = sum(member)
    if count < 4:
        return None
    cnt = float(count)
    s = _lane_tree(n, member, lambda i: (float(x0[i]), float(y0[i]), float(x1[i]), float(y1[i])), 4)
    c0x, c0y, c1x, c1y = s[0] / cnt, s[1] / cnt, s[2] / cnt, s[3] / cnt

    def dist(i):
        dx0, dy0, dx1, dy1 = float(x0[i]) - c0x, float(y0[i]) - c0y, float(x1[i]) - c1x, float(y1[i]) - c1y
        return math.sqrt(dx0 * dx0 + dy0 * dy0), math.sqrt(dx1 * dx1 + dy1 * dy1)
    d = _lane_tree(n, member, dist, 2)
    d0, d1 = d[0] / cnt, d[1] / cnt
    if not d0 > 0.0 or not d1 > 0.0:
        return None
    s0, s1 = 1.4142135623730951 / d0, 1.4142135623730951 / d1

    def terms(i):
        x, y = s0 * (float(x0[i]) - c0x), s0 * (float(y0[i]) - c0y)
        u, v = s1 * (float(x1[i]) - c1x), s1 * (float(y1[i]) - c1y)
        a = [x * x, x * y, x, y * y, y, 1.0]
        w = u * u + v * v
        return a + [u * e for e in a] + [v * e for e in a] + [w * e for e in a]
    t = _lane_tree(n, member, terms, 24)
    sym = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    m = [[0.0] * 9 for _ in range(9)]
    for i in range(3):
        for j in range(3):
            k = sym[i][j]
            m[i][j] = m[3 + i][3 + j] = t[k]
            m[i][6 + j] = m[6 + i][j] = -t[6 + k]
            m[3 + i][6 + j] = m[6 + i][3 + j] = -t[12 + k]
            m[6 + i][6 + j] = t[18 + k]
    for _ in range(60):
        rotated = False
        for p in range(9):
            for q in range(p + 1, 9):
                rotated = _py_jacobi_pair(m, p, q) or rotated
        if not rotated:
            break
    norms = [_py_norm(r) for r in m]
    mi = 0
    for i in range(1, 9):
        if norms[i] < norms[mi]:
            mi = i
    if mi != 8:
        m[mi] = list(m[8])
    e = float(EPS_MODEL)
    threshold = (e * e) * (cnt * 0.25)
    if not all(_py_norm(m[i]) > threshold for i in range(8)):
        return None
    best, best_n = [0.0] * 9, -1.0
    for k in range(9):
        nv = [1.0 if j == k else 0.0 for j in range(9)]
        for i in range(8):
            r = m[i]
            nr = 0.0
            for j in range(9):
                nr += r[j] * r[j]
            c = r[k] * (1.0 / nr)
            nv = [nv[j] - c * r[j] for j in range(9)]
        nn = 0.0
        for j in range(9):
            nn += nv[j] * nv[j]
        if nn > best_n:
            best_n, best = nn, nv
    if not best_n > 0.0:
        return None
    bn = math.sqrt(best_n)
    hn = [b / bn for b in best]
    tx0, ty0 = -(s0 * c0x), -(s0 * c0y)
    a = [0.0] * 9
    for r in range(3):
        a[3 * r] = hn[3 * r] * s0
        a[3 * r + 1] = hn[3 * r + 1] * s0
        a[3 * r + 2] = (hn[3 * r] * tx0 + hn[3 * r + 1] * ty0) + hn[3 * r + 2]
    is1 = 1.0 / s1
    hh = [0.0] * 9
    for col in range(3):
        hh[col] = a[col] * is1 + c1x * a[6 + col]
        hh[3 + col] = a[3 + col] * is1 + c1y * a[6 + col]
        hh[6 + col] = a[6 + col]
    fro = 0.0
    for j in range(9):
        fro += hh[j] * hh[j]
    fro = math.sqrt(fro)
    if not abs(hh[8]) > 1e-12 * fro:
        return None
    return np.array([hh[j] / hh[8] for j in range(9)], np.float64).astype(np.float32)


def py_refine(k0, k1, m, h_in, eps, max_it):
    """the loop of the statement -> (member mask, H as 9 float32, accepted fits)"""
    x0, y0 = k0["x"][m["index_0"]].astype(np.float32), k0["y"][m["index_0"]].astype(np.float32)
    x1, y1 = k1["x"][m["index_1"]].astype(np.float32), k1["y"][m["index_1"]].astype(np.float32)
    n = len(m)

    def classify(h):
        return [_py_inlier(h, x0[i], y0[i], x1[i], y1[i], eps) for i in range(n)]
    h = np.asarray(h_in, np.float32).reshape(9).copy()
    member = classify(h)
    done = 0
    while done < max_it:
        h2 = _py_fit(x0, y0, x1, y1, member)
        if h2 is None:
            break
        nxt = classify(h2)
        if sum(nxt) < sum(member):
            break
        grew = sum(nxt) > sum(member)
        h, member, done = h2, nxt, done + 1
        if not grew:
            break
    return np.array(member, bool), h, done


def _order_case(amd, n, inlier_positions, seed):
    """n matches whose inliers of H_true (noise 0.3 px) sit exactly at inlier_positions; the others are displaced >= 50 px"""
    rng = np.random.default_rng(seed)
    h = _h_true(rng)
    p0 = _points(rng, h, n)
    inl = np.zeros(n, bool)
    inl[list(inlier_positions)] = True
    p1 = _apply(h, p0) + rng.normal(0, 0.3, (n, 2))
    ang = rng.uniform(0, 2 * np.pi, n)
    p1[~inl] += (np.c_[np.cos(ang), np.sin(ang)] * rng.uniform(50, 400, n)[:, None])[~inl]
    k0, k1, m = _kp(amd, p0), _kp(amd, p1.astype(np.float32)), _ident_matches(amd, n)
    assert np.array_equal(inlier_rule(h, k0, k1, m, 3.0), inl)
    return k0, k1, m, h.astype(np.float32)


ORDER_CASES = {
    "257, inliers at 0 mod 256": (257, range(0, 257, 256)),
    "513, inliers at 0 mod 256": (513, range(0, 513, 256)),
    "2049, inliers at 0 mod 256": (2049, range(0, 2049, 256)),     # nine inliers, all of lane 0: one lane adds them in order
    "1300, inliers at 0 and 255 mod 256": (1300, [i for i in range(1300) if i % 256 in (0, 255)]),
    "600, one non-inlier at 255": (600, [i for i in range(600) if i != 255]),
    "256, all": (256, range(256)),
    "300, every third": (300, range(1, 300, 3)),
}


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_summation_order(amd, name):
    """Host result = the Python restatement with the documented lane / tree order, bit for bit on H (and the list, the count of
    fits).  The first two lists are the issue's: their two and three inliers are fewer than a fit takes, so both sides
    return h_in; the others reach the sums with members in one lane only, in the first and the last lane, with a hole at
    the last lane, with exactly one element per lane, and with members spread over every lane."""
    n, pos = ORDER_CASES[name]
    k0, k1, m, h_in = _order_case(amd, n, pos, 77 + n)
    for max_it in (1, 3):
        kept, h, its = amd.refine_homography(k0, k1, m, h_in, 3.0, max_it)
        mask, hp, itp = py_refine(k0, k1, m, h_in, 3.0, max_it)
        assert its == itp, (name, its, itp)
        assert np.array_equal(h.reshape(9).view(np.uint32), hp.view(np.uint32)), (name, h, hp)
        assert np.array_equal(kept, m[mask])
        if len(list(pos)) >= 4:
            assert its >= 1, name
        else:
            assert its == 0 and np.array_equal(h.reshape(9).view(np.uint32), h_in.reshape(9).view(np.uint32))


def test_python_restatement_on_the_noisy_cases(amd, noisy):
    for seed in (0, 3):
        k0, k1, m, _, _, h_in = noisy[seed]
        kept, h, its = amd.refine_homography(k0, k1, m, h_in, 3.0, 8)
        mask, hp, itp = py_refine(k0, k1, m, h_in, 3.0, 8)
        assert its == itp and np.array_equal(h.reshape(9).view(np.uint32), hp.view(np.uint32)) and np.array_equal(kept, m[mask])


# ---- refusals and declarations -------------------------------------------------------------------------------------------
def test_refusals(amd):
    L, bad = amd.lib(), _status(amd)
    k0, k1, m, h = _order_case(amd, 20, range(20), 5)
    out = np.zeros(20, amd.MATCH_DTYPE)
    n = C.c_uint64(12345)
    hout = np.full(9, 7.0, np.float32)
    it = C.c_uint32(99)
    hin = np.ascontiguousarray(h.reshape(9))
    fp = C.POINTER(C.c_float)

    def call(k0p=k0.ctypes.data, n0=len(k0), k1p=k1.ctypes.data, n1=len(k1), mp=m.ctypes.data, nm=len(m),
             hp=hin.ctypes.data_as(fp), eps=3.0, outp=out.ctypes.data, np_=C.byref(n)):
        return L.akz_refine_homography(k0p, n0, k1p, n1, mp, nm, hp, eps, 8, outp, np_, hout.ctypes.data_as(fp), C.byref(it))
    assert call(np_=None) == bad
    assert call(mp=None) == bad
    assert call(outp=None) == bad
    assert call(hp=None) == bad
    for eps in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert call(eps=eps) == bad, eps
    assert call(n0=19) == bad and call(n1=19) == bad      # an index out of range
    assert call(k0p=None) == bad and call(k1p=None) == bad
    # nothing was written by a refused call
    assert n.value == 12345 and it.value == 99 and np.all(hout == 7.0) and not out.view(np.uint8).any()
    # NULL h_out and iterations are allowed; an empty list is AKZ_OK
    assert L.akz_refine_homography(k0.ctypes.data, len(k0), k1.ctypes.data, len(k1), m.ctypes.data, len(m), hin.ctypes.data_as(fp), 3.0,
                                   8, out.ctypes.data, C.byref(n), None, None) == 0
    assert n.value == 20
    assert L.akz_refine_homography(None, 0, None, 0, None, 0, hin.ctypes.data_as(fp), 3.0, 8, None, C.byref(n), None, None) == 0
    assert n.value == 0


def test_symbols_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    for name in ("akz_refine_homography", "akz_match_features_homography_refined", "akz_match_features_homography_refined_pairs",
                 "akz_match_features_homography_refined_guided", "akz_match_features_homography_refined_guided_pairs"):
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert L.akz_abi_version() == 6
    assert "no refit" not in hdr
    for name in ("refine_homography", "match_features_homography_refined", "match_features_homography_refined_guided",
                 "match_features_homography_refined_pairs", "match_features_homography_refined_guided_pairs"):
        assert callable(getattr(amd, name)), name
    for name in ("match_features_homography_refined_pairs", "match_features_homography_refined_guided_pairs"):
        assert callable(getattr(amd.Context, name)), name
