"""The homography RANSAC on the host (no GPU): its 4-index draws against the plain `%` loop, the model against an independent
numpy statement (np.linalg.svd null vector of the same normalised design matrix), the degeneracy rules, the exact inlier set
on synthetic correspondences, and the edge cases.  The reference has no homography: these, and the host / device agreement
of tests/test_gpu_homography.py, are its correctness argument."""
import ctypes as C

import numpy as np
import pytest

from test_match_pairs_host import _color, _status, _xorshift

N_VALUES = [4, 5, 7, 8, 9, 10, 16, 64, 1024, 1 << 20, 1 << 31, (1 << 31) - 1, (1 << 32) + 1, (1 << 40) + 12345,
            0xFFFFFFFFFFFFFFC5, 0x9E3779B97F4A7C15, (1 << 63) + 1, (1 << 64) - 1, 3 * (1 << 62) + 7]


def _plain_draws_k(s0, s1, n, trials, k):
    src = _xorshift(s0, s1)
    out = []
    for _ in range(trials):
        picked = []
        while len(picked) < k:
            j = next(src) % n
            if j not in picked:
                picked.append(j)
        out.extend(sorted(picked))
    return np.array(out, np.uint64)


def _draws(amd, s0, s1, n, trials, k):
    got = np.zeros(max(1, trials * k), np.uint64)
    st = amd.lib().akz_debug_ransac_samples_k(s0, s1, n, trials, k, got.ctypes.data_as(C.POINTER(C.c_uint64)))
    return st, got[:trials * k]


@pytest.mark.parametrize("n", N_VALUES)
def test_four_index_draws_equal_the_plain_modulo_loop(amd, n):
    trials = 40 if n < 64 else 300
    for s0, s1 in ((42, 69), (1, 2), (0xDEADBEEFCAFEF00D, 0x0123456789ABCDEF)):
        st, got = _draws(amd, s0, s1, n, trials, 4)
        assert st == 0
        assert np.array_equal(got, _plain_draws_k(s0, s1, n, trials, 4)), (n, s0, s1)


@pytest.mark.parametrize("n", [8, 9, 64, 1 << 31, (1 << 64) - 1])
def test_eight_index_draws_are_unchanged(amd, n):
    exp = np.zeros(300 * 8, np.uint64)
    assert amd.lib().akz_debug_ransac_samples(42, 69, n, 300, exp.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    st, got = _draws(amd, 42, 69, n, 300, 8)
    assert st == 0 and np.array_equal(got, exp)


def test_draw_refusals(amd):
    bad = _status(amd)
    for n, k in ((3, 4), (7, 8), (0, 4), (100, 5), (100, 0)):
        st, _ = _draws(amd, 42, 69, n, 3, k)
        assert st == bad, (n, k)


# ---- the model against numpy ---------------------------------------------------------------------------------------------
def _normalise(p):
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    s = np.sqrt(2.0) / d
    return s * (p - c), c, s


def numpy_homography(p0, p1):
    """The model of include/akaze_hip.h stated with numpy in f64: Hartley normalisation, the 8 x 9 design matrix, the null
    vector from np.linalg.svd, denormalised and scaled to H[2, 2] = 1.  Returns (H, condition number of the 8 nonzero
    singular values of the normalised design matrix)."""
    q0, c0, s0 = _normalise(np.asarray(p0, np.float64))
    q1, c1, s1 = _normalise(np.asarray(p1, np.float64))
    rows = []
    for (x, y), (u, v) in zip(q0, q1):
        rows.append([-x, -y, -1, 0, 0, 0, u * x, u * y, u])
        rows.append([0, 0, 0, -x, -y, -1, v * x, v * y, v])
    a = np.array(rows)
    _, sv, vt = np.linalg.svd(a)
    hn = vt[-1].reshape(3, 3)
    t0 = np.array([[s0, 0, -s0 * c0[0]], [0, s0, -s0 * c0[1]], [0, 0, 1]])
    t1inv = np.array([[1 / s1, 0, c1[0]], [0, 1 / s1, c1[1]], [0, 0, 1]])
    h = t1inv @ hn @ t0
    return h / h[2, 2], sv[0] / sv[7]


def _kp(amd, pts):
    k = np.zeros(len(pts), amd.KEYPOINT_DTYPE)
    k["x"] = pts[:, 0]
    k["y"] = pts[:, 1]
    return k


def _ident_matches(amd, n):
    m = np.zeros(n, amd.MATCH_DTYPE)
    m["index_0"] = np.arange(n)
    m["index_1"] = np.arange(n)
    return m


def _apply(h, p):
    q = np.c_[p, np.ones(len(p))] @ np.asarray(h, np.float64).T
    return q[:, :2] / q[:, 2:]


def test_model_equals_numpy(amd):
    """Within 1e-4 relative per entry wherever the normalised design matrix has a condition number below 1e4: the model is an
    f64 result rounded to f32 (~6e-8 relative) and the f64 error is at most ~cond * 2^-52 (~1e-12); 1e-4 leaves three orders
    of magnitude for rounding through the denormalisation.  The four sample points transfer onto their partners within 1e-3
    px at coordinates up to 4096, by the same argument."""
    rng = np.random.default_rng(7)
    compared = transferred = 0
    for it in range(400):
        p0 = rng.uniform(0, 4096, (4, 2)).astype(np.float32)
        if it % 2:  # strongly projective maps
            p1 = (p0 + rng.uniform(-400, 400, (4, 2))).astype(np.float32)
        else:       # near a similarity
            a, sc = rng.uniform(-0.3, 0.3), rng.uniform(0.8, 1.2)
            rot = sc * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            p1 = (p0 @ rot.T + rng.uniform(-200, 200, 2) + rng.uniform(-20, 20, (4, 2))).astype(np.float32)
        h = amd.estimate_homography(_kp(amd, p0), _kp(amd, p1), _ident_matches(amd, 4), amd.HOMOGRAPHY_EPSILON_MODEL)
        exp, cond = numpy_homography(p0.astype(np.float64), p1.astype(np.float64))
        if cond >= 1e4:
            continue
        q0, q1 = _normalise(p0.astype(np.float64))[0], _normalise(p1.astype(np.float64))[0]
        tri = [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]

        def cross(q, t):
            a, b, c = q[list(t)]
            return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        degenerate = any(abs(cross(q0, t)) <= 1e-9 or abs(cross(q1, t)) <= 1e-9 or (cross(q0, t) > 0) != (cross(q1, t) > 0)
                         for t in tri)
        if degenerate:
            assert h is None, it
            continue
        assert h is not None, it
        assert h.dtype == np.float32 and h[2, 2] == 1.0
        rel = np.abs(h.astype(np.float64) - exp) / np.abs(exp)
        print(it, "cond", cond, "max rel", rel.max())
        assert np.all(np.abs(h.astype(np.float64) - exp) <= 1e-4 * np.abs(exp)), (it, h, exp)
        compared += 1
        # The transfer bound rests on the output rounding: an f32 entry moves by up to 2^-24 of itself, which moves H p0 by
        # up to rb = 2^-24 (|h0 x| + |h1 y| + |h2| + |u| (|h6 x| + |h7 y| + |h8|)) / |w| (first order, numpy's H).  Where rb is
        # below 5e-4 px (w not near 0: the map does not send a sample point towards infinity; ~4.9e-4 for the identity at
        # 4096) the 1e-3 px bound leaves as much again for the f64 error and the rounding of the denormalisation.
        p0d, p1d = p0.astype(np.float64), p1.astype(np.float64)
        w = p0d @ exp[2, :2] + exp[2, 2]
        mag = np.abs(p0d[:, None, :] * exp[None, :, :2]).sum(axis=2) + np.abs(exp[:, 2])[None, :]
        rb = 2.0 ** -24 * (mag[:, :2] + np.abs(_apply(exp, p0d)) * mag[:, 2:]) / np.abs(w)[:, None]
        if rb.max() < 5e-4:
            err = np.abs(_apply(h, p0d) - p1d).max()
            print(it, "transfer", err, "rounding bound", rb.max())
            assert err < 1e-3, (it, err)
            transferred += 1
    assert compared >= 100 and transferred >= 50, (compared, transferred)


def test_degenerate_samples_give_no_model(amd):
    eps = amd.HOMOGRAPHY_EPSILON_MODEL
    m4 = _ident_matches(amd, 4)
    good0 = np.array([[100, 100], [900, 120], [880, 700], [130, 650]], np.float32)
    good1 = good0 + np.array([[5, 3], [-4, 8], [6, -2], [1, 1]], np.float32)
    assert amd.estimate_homography(_kp(amd, good0), _kp(amd, good1), m4, eps) is not None
    line = good0.copy()
    line[2] = [500, 110]                   # on the line through points 0 and 1
    assert amd.estimate_homography(_kp(amd, line), _kp(amd, good1), m4, eps) is None
    assert amd.estimate_homography(_kp(amd, good0), _kp(amd, line), m4, eps) is None
    flipped = good1.copy()
    flipped[[0, 1]] = flipped[[1, 0]]      # points 0 and 1 swapped in image 1: triple (0, 1, 2) changes orientation
    assert amd.estimate_homography(_kp(amd, good0), _kp(amd, flipped), m4, eps) is None
    mirror = good1 * np.array([-1, 1], np.float32) + np.array([1000, 0], np.float32)  # every triple flipped
    assert amd.estimate_homography(_kp(amd, good0), _kp(amd, mirror), m4, eps) is None
    same = good0.copy()
    same[3] = same[1]                      # two identical points
    assert amd.estimate_homography(_kp(amd, same), _kp(amd, good1), m4, eps) is None
    assert amd.estimate_homography(_kp(amd, good1), _kp(amd, same), m4, eps) is None


# ---- the exact outcome on synthetic correspondences ----------------------------------------------------------------------
def synthetic_case(amd, seed):
    """A projective H_true (rotation, scale 0.7..1.4, perspective up to 3e-4, translation up to 300 px), 400..2 000 matches,
    inliers p1 = H_true p0 (f64, rounded to f32), outliers displaced at least 50 px from H_true p0, inlier share 0.5..0.9.
    Returns (k0, k1, matches, inlier mask, H_true)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(400, 2001))
    share = rng.uniform(0.5, 0.9)
    a, sc = rng.uniform(-np.pi, np.pi), rng.uniform(0.7, 1.4)
    h = np.array([[sc * np.cos(a), -sc * np.sin(a), rng.uniform(-300, 300)],
                  [sc * np.sin(a), sc * np.cos(a), rng.uniform(-300, 300)],
                  [rng.uniform(-3e-4, 3e-4), rng.uniform(-3e-4, 3e-4), 1.0]])
    # image 0 points where H_true keeps w > 0.2 (a plane seen from its front)
    p0 = np.zeros((0, 2))
    while len(p0) < n:
        c = rng.uniform([0, 0], [1920, 1080], (n, 2))
        w = c @ h[2, :2] + 1.0
        p0 = np.r_[p0, c[w > 0.2]]
    p0 = p0[:n].astype(np.float32).astype(np.float64)
    inl = rng.uniform(size=n) < share
    p1 = _apply(h, p0)
    ang = rng.uniform(0, 2 * np.pi, n)
    dist = rng.uniform(50, 400, n)
    p1[~inl] += np.c_[np.cos(ang), np.sin(ang)][~inl] * dist[~inl, None]
    p1 = p1.astype(np.float32)
    assert np.all(np.hypot(*(p1.astype(np.float64) - _apply(h, p0))[~inl].T) >= 50.0 - 1e-3)
    # keypoint lists in an order of their own, the matches pointing into them
    perm0, perm1 = rng.permutation(n), rng.permutation(n)
    k0 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k1 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k0["x"][perm0], k0["y"][perm0] = p0[:, 0], p0[:, 1]
    k1["x"][perm1], k1["y"][perm1] = p1[:, 0], p1[:, 1]
    m = np.zeros(n, amd.MATCH_DTYPE)
    m["index_0"], m["index_1"] = perm0, perm1
    m["distance"] = rng.uniform(0, 100, n)
    return k0, k1, m, inl, h


@pytest.mark.parametrize("seed", range(6))
def test_exact_inlier_set_on_synthetic_correspondences(amd, seed):
    """The winner keeps exactly the true inliers: at a share >= 0.5 the chance that 1 000 trials draw no all-inlier sample is
    below (15/16)^1000 ~ 1e-28, an all-inlier model errs far below eps = 2 px, and no wrong model gathers half the matches."""
    k0, k1, m, inl, _ = synthetic_case(amd, seed)
    amd.random_seed(42, 69)
    kept, h = amd.remove_outliers_homography(k0, k1, m, 1000, amd.HOMOGRAPHY_EPSILON_MODEL, 2.0)
    assert h is not None
    assert np.array_equal(kept, m[inl]), (len(kept), int(inl.sum()))


def test_edge_cases(amd):
    k0, k1, m, inl, _ = synthetic_case(amd, 11)
    eps_m = amd.HOMOGRAPHY_EPSILON_MODEL
    # fewer than 4 matches: unchanged, nothing drawn
    amd.random_seed(42, 69)
    fresh = _color(amd)
    for n in range(4):
        amd.random_seed(42, 69)
        kept, h = amd.remove_outliers_homography(k0, k1, m[:n], 1000, eps_m, 2.0)
        assert np.array_equal(kept, m[:n]) and h is None
        assert _color(amd) == fresh
    # 4 matches draw
    amd.random_seed(42, 69)
    amd.remove_outliers_homography(k0, k1, m[:4], 10, eps_m, 2.0)
    assert _color(amd) != fresh
    # 0 trials: everything kept, no model
    kept, h = amd.remove_outliers_homography(k0, k1, m, 0, eps_m, 2.0)
    assert np.array_equal(kept, m) and h is None
    # eps 0: no model has an inlier -> everything kept, no model
    kept, h = amd.remove_outliers_homography(k0, k1, m, 50, eps_m, 0.0)
    assert np.array_equal(kept, m) and h is None
    # an index out of range
    bad = m.copy()
    bad["index_1"][7] = len(k1)
    with pytest.raises(amd.AkazeError) as e:
        amd.remove_outliers_homography(k0, k1, bad, 10, eps_m, 2.0)
    assert e.value.status == _status(amd)
    bad4 = m[:4].copy()
    bad4["index_0"][2] = len(k0)
    with pytest.raises(amd.AkazeError) as e:
        amd.estimate_homography(k0, k1, bad4, eps_m)
    assert e.value.status == _status(amd)


def test_symbols_declared(amd):
    L = amd.lib()
    for name in ("akz_estimate_homography", "akz_remove_outliers_homography", "akz_match_features_homography",
                 "akz_match_features_homography_pairs", "akz_debug_ransac_samples_k"):
        assert hasattr(L, name) and name in L._declared, name
    assert L.akz_abi_version() == 6
