"""The relative pose behind a fundamental matrix on the host (akz_recover_pose_host; no GPU call): declarations and refusals,
the statement against an independent numpy statement (tests/pose_numpy.py) and against the truth of noise-free two-view scenes,
the candidate order and the tie rule on a hand-made E, the cases without a pose, the filter and the triangulated points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_numpy as pn
from test_homography_host import _ident_matches, _kp
from test_match_pairs_host import ROOT, _status

NEW_SYMBOLS = ("akz_recover_pose_host", "akz_match_features_seeded_pose_pairs")
# distinct cameras, fx != fy, principal points off the centre: a shared K would hide a K0 / K1 mix-up
CAMS = ((1180.0, 1230.0, 940.0, 560.0), (1250.0, 1190.0, 985.0, 520.0))
SIZES = (8, 9, 255, 256, 257, 1000)
SEEDS = range(6)


def scene_case(amd, seed, n, **kw):
    """-> (k0, k1, identity matches, scene) with the coordinates rounded to f32 as the library sees them"""
    kw.setdefault("cams", CAMS)
    sc = pn.pose_scene(seed, n, **kw)
    return _kp(amd, sc["p0"].astype(np.float32)), _kp(amd, sc["q1"].astype(np.float32)), _ident_matches(amd, n), sc


def reference(amd, k0, k1, m, f, pose, cams=CAMS):
    """the numpy statement on the same list, its free sign taken from the library's +t (see pose_numpy)"""
    plus_t = None
    if pose.found:
        plus_t = pose.T.astype(np.float64) * (1.0 if pose.winner % 2 == 0 else -1.0)
    p0 = np.c_[k0["x"][m["index_0"]], k0["y"][m["index_0"]]]
    p1 = np.c_[k1["x"][m["index_1"]], k1["y"][m["index_1"]]]
    return pn.numpy_pose(p0, p1, f, cams[0], cams[1], like_t=plus_t)


# ---- declarations and refusals ---------------------------------------------------------------------------------------------
def test_symbols_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert L.akz_abi_version() == 6
    assert "typedef struct akz_camera" in hdr and "typedef struct akz_pose" in hdr
    assert C.sizeof(amd.Pose) == 84 and C.sizeof(amd.Camera) == 32   # 21 four-byte fields; four doubles
    assert C.sizeof(amd.RansacOptions) == 80
    for name in ("Camera", "Pose", "recover_pose_host", "match_features_seeded_pose", "match_features_seeded_pose_pairs"):
        assert callable(getattr(amd, name)), name
    assert callable(amd.Context.match_features_seeded_pose_pairs)


def test_refusals(amd):
    L, bad = amd.lib(), _status(amd)
    k0, k1, m, sc = scene_case(amd, 5, 20)
    out = np.zeros(20, amd.MATCH_DTYPE)
    n = C.c_uint64(12345)
    pose = amd.Pose()
    C.memset(C.byref(pose), 0x5A, C.sizeof(pose))
    pts = np.full(60, 7.0, np.float32)
    f = np.ascontiguousarray(sc["f"].astype(np.float32).reshape(9))
    fp = C.POINTER(C.c_float)
    c0, c1 = amd.Camera(*CAMS[0]), amd.Camera(*CAMS[1])

    def call(k0p=k0.ctypes.data, n0=len(k0), k1p=k1.ctypes.data, n1=len(k1), mp=m.ctypes.data, nm=len(m), f_p=f.ctypes.data_as(fp),
             cam0=C.byref(c0), cam1=C.byref(c1), outp=out.ctypes.data, np_=C.byref(n), pose_p=C.byref(pose)):
        return L.akz_recover_pose_host(k0p, n0, k1p, n1, mp, nm, f_p, cam0, cam1, outp, np_, pose_p, pts.ctypes.data_as(fp))
    # those of akz_refine_fundamental_matrix for the keypoint and match arguments
    assert call(np_=None) == bad and call(mp=None) == bad and call(outp=None) == bad
    assert call(n0=19) == bad and call(n1=19) == bad
    assert call(k0p=None) == bad and call(k1p=None) == bad
    # its own
    assert call(f_p=None) == bad and call(cam0=None) == bad and call(cam1=None) == bad and call(pose_p=None) == bad
    for field in ("fx", "fy"):
        for which in (0, 1):
            cam = amd.Camera(*CAMS[which])
            setattr(cam, field, 0.0)
            assert call(**{f"cam{which}": C.byref(cam)}) == bad, (field, which)
    for field in ("fx", "fy", "cx", "cy"):
        for v in (float("nan"), float("inf"), float("-inf")):
            cam = amd.Camera(*CAMS[1])
            setattr(cam, field, v)
            assert call(cam1=C.byref(cam)) == bad, (field, v)
    # nothing was written by a refused call
    assert n.value == 12345 and bytes(pose) == b"\x5a" * 84 and np.all(pts == 7.0) and not out.view(np.uint8).any()
    # an empty list is AKZ_OK with found 0; NULL points is allowed
    assert L.akz_recover_pose_host(None, 0, None, 0, None, 0, f.ctypes.data_as(fp), C.byref(c0), C.byref(c1), None, C.byref(n), C.byref(pose),
                                   None) == 0
    assert n.value == 0 and pose.found == 0 and pose.winner == 0 and not pose.R.any() and not pose.T.any() and not pose.counts.any()
    assert call() == 0 and n.value == 20 and pose.found == 1


# ---- against numpy and the truth ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact(amd):
    """the 36 noise-free scenes with the true F rounded to f32, the library's result and the numpy statement's (built once, left
    unchanged)"""
    res = []
    for n in SIZES:
        for seed in SEEDS:
            k0, k1, m, sc = scene_case(amd, 100 * n + seed, n)
            f = sc["f"].astype(np.float32)
            kept, pose, pts = amd.recover_pose_host(k0, k1, m, f, *CAMS, points=True)
            res.append((n, seed, sc, m, kept, pose, pts, reference(amd, k0, k1, m, f, pose)))
    return res


def test_pose_equals_numpy_and_the_truth(exact):
    """Winner and counts are exact.  R and t as ||R - R'||_F and ||t - t'|| (not arccos: its resolution near 0 is 2e-8), worst over
    the 36 scenes, measured on this statement:
        numpy statement to the truth      R 6.9e-8   t 3.8e-8    (the f32 rounding of F and nothing else)
        this library to the numpy one     R 4.5e-8   t 3.6e-8    (the f32 rounding of the result)
    The bound is ten times the larger figure of each column: R 6.9e-7, t 3.8e-7.  sigma[] equals numpy's singular values to 1e-7 (sigma2 / sigma1 is
    1 to f32; sigma3 / sigma1, the f32 rounding of F seen through K0 and K1, stays below 1e-7)."""
    worst = dict(R_numpy_truth=0.0, t_numpy_truth=0.0, R_lib_numpy=0.0, t_lib_numpy=0.0, R_lib_truth=0.0, t_lib_truth=0.0)
    for n, seed, sc, m, kept, pose, pts, ref in exact:
        what = (n, seed)
        assert pose.found == 1 and ref["found"] == 1, what
        assert [int(v) for v in pose.counts] == [int(v) for v in ref["in_front"]], (what, pose.counts, ref["in_front"])
        assert pose.winner == ref["winner"] and pose.counts[pose.winner] == n, (what, pose.winner, pose.counts)
        assert sorted(int(v) for v in pose.counts) == [0, 0, 0, n], (what, pose.counts)
        assert np.array_equal(kept, m), what
        assert abs(float(pose.singular_values[1]) - 1.0) < 1e-6, (what, pose.singular_values)
        assert np.allclose(pose.singular_values, ref["sigma"], atol=1e-7), what
        tt = sc["t"] / np.linalg.norm(sc["t"])
        r, t = pose.R.astype(np.float64), pose.T.astype(np.float64)
        for key, v in (("R_numpy_truth", np.linalg.norm(ref["r"] - sc["r"])), ("t_numpy_truth", np.linalg.norm(ref["t"] - tt)),
                       ("R_lib_numpy", np.linalg.norm(r - ref["r"])), ("t_lib_numpy", np.linalg.norm(t - ref["t"])),
                       ("R_lib_truth", np.linalg.norm(r - sc["r"])), ("t_lib_truth", np.linalg.norm(t - tt))):
            worst[key] = max(worst[key], float(v))
    print("pose figures:", {k: f"{v:.2e}" for k, v in worst.items()})
    bound_r, bound_t = 6.9e-7, 3.8e-7
    assert worst["R_lib_numpy"] <= bound_r and worst["R_lib_truth"] <= bound_r, worst
    assert worst["t_lib_numpy"] <= bound_t and worst["t_lib_truth"] <= bound_t, worst


def test_points_are_the_scene(exact):
    """The points against X_true / |t_true| (camera 0's frame, |t| = 1) on the noise-free scenes, as the largest |difference| of a
    coordinate, worst over the 36 scenes, measured on this statement:
        numpy statement to the truth      4.0e-5   (the f32 rounding of F and of the coordinates, at depths of 4 .. 24 baselines)
        this library to the numpy one     9.6e-7   (the f32 rounding of a coordinate of up to 16)
    The bound is ten times the larger: 4.0e-4."""
    worst = dict(numpy_truth=0.0, lib_numpy=0.0, lib_truth=0.0)
    for n, seed, sc, m, kept, pose, pts, ref in exact:
        truth = sc["x"] / np.linalg.norm(sc["t"])
        assert pts.shape == (n, 3) and pts.dtype == np.float32 and ref["points"].shape == (n, 3), (n, seed)
        for key, v in (("numpy_truth", np.abs(ref["points"] - truth).max()), ("lib_numpy", np.abs(pts - ref["points"]).max()),
                       ("lib_truth", np.abs(pts - truth).max())):
            worst[key] = max(worst[key], float(v))
    print("point figures:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["lib_numpy"] <= 4.0e-4 and worst["lib_truth"] <= 4.0e-4, worst


# ---- candidate order and ties ----------------------------------------------------------------------------------------------------
UNIT = (1.0, 1.0, 0.0, 0.0)  # pixels are normalised coordinates: F is E
V = np.array([[0.6, -0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]], np.float32).astype(np.float64)  # columns v1, v2, v3 (as f32 holds them)
W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def hand_made():
    """E = diag(1, 1, 0) V^T: its rows are orthogonal already (v1 . v2 is exactly 0 in f64) and of equal norm, so the rotations
    leave them alone, row 0 is sigma1 v1^T (the first among equals), U is the identity, u3 = +z.  -> (E, the four candidates)"""
    e = np.diag([1.0, 1.0, 0.0]) @ V.T
    ra, rb, t = W @ V.T, W.T @ V.T, np.array([0.0, 0.0, 1.0])
    return e.astype(np.float32), [(ra, t), (ra, -t), (rb, t), (rb, -t)]


def views(amd, r, t, n, seed):
    """n points in front of both cameras of (identity, (r, t)) -> (p0, p1) in normalised coordinates, f64"""
    rng = np.random.default_rng(seed)
    x = np.c_[rng.uniform(-4, 4, n), rng.uniform(-2.5, 2.5, n), rng.uniform(4, 12, n)]
    y = x @ r.T + t
    assert (y[:, 2] > 0).all()
    return x[:, :2] / x[:, 2:], y[:, :2] / y[:, 2:]


@pytest.mark.parametrize("winner", [0, 1, 2, 3])
def test_each_candidate_wins_in_turn(amd, winner):
    e, cand = hand_made()
    r, t = cand[winner]
    p0, p1 = views(amd, r, t, 40, 10 + winner)
    kept, pose = amd.recover_pose_host(_kp(amd, p0.astype(np.float32)), _kp(amd, p1.astype(np.float32)), _ident_matches(amd, 40), e, UNIT, UNIT)
    counts = [0, 0, 0, 0]
    counts[winner] = 40
    assert pose.found == 1 and pose.winner == winner and [int(v) for v in pose.counts] == counts, (pose.winner, pose.counts)
    assert np.array_equal(pose.R, r.astype(np.float32)) and np.array_equal(pose.T, t.astype(np.float32)), (pose.R, r)
    assert len(kept) == 40


@pytest.mark.parametrize("first,second", [(0, 2), (2, 0), (1, 3), (3, 1), (0, 1), (3, 2)])
def test_equal_counts_keep_the_first_candidate(amd, first, second):
    """the matches of two candidates' scenes in one list, `first`'s in front: the lower index wins whichever comes first"""
    e, cand = hand_made()
    a0, a1 = views(amd, *cand[first], 12, 50 + first)
    b0, b1 = views(amd, *cand[second], 12, 60 + second)
    k0, k1 = _kp(amd, np.r_[a0, b0].astype(np.float32)), _kp(amd, np.r_[a1, b1].astype(np.float32))
    m = _ident_matches(amd, 24)
    kept, pose = amd.recover_pose_host(k0, k1, m, e, UNIT, UNIT)
    counts = [0, 0, 0, 0]
    counts[first] = counts[second] = 12
    assert [int(v) for v in pose.counts] == counts and pose.found == 1 and pose.winner == min(first, second), (pose.winner, pose.counts)
    mine = np.arange(12) if pose.winner == first else np.arange(12, 24)
    assert np.array_equal(kept, m[mine])


# ---- no pose -----------------------------------------------------------------------------------------------------------------
def test_no_pose(amd):
    k0, k1, m, sc = scene_case(amd, 3, 12)
    f = sc["f"].astype(np.float32)

    def unchanged(kk0, kk1, mm, ff, cams, sigma):
        kept, pose, pts = amd.recover_pose_host(kk0, kk1, mm, ff, *cams, points=True)
        assert pose.found == 0 and pose.winner == 0 and not pose.R.any() and not pose.T.any(), ff
        assert np.array_equal(kept, mm) and pts is None
        assert sigma(pose.singular_values), pose.singular_values
        return pose
    # a zero F: nothing was computed
    p = unchanged(k0, k1, m, np.zeros(9, np.float32), CAMS, lambda s: not s.any())
    assert not p.counts.any()
    # a rank-1 F: sigma2 / sigma1 is at rounding level
    p = unchanged(k0, k1, m, np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]).astype(np.float32), CAMS, lambda s: s[0] == 1.0 and s[1] < 1e-6)
    assert not p.counts.any()
    # every match behind under every candidate: the rays (0, 0, 1) <-> (0, 0, 1) are parallel under both rotations about z
    e, _ = hand_made()
    z = _kp(amd, np.zeros((9, 2), np.float32))
    p = unchanged(z, z, _ident_matches(amd, 9), e, (UNIT, UNIT), lambda s: s[0] == 1.0 and s[1] == 1.0 and s[2] == 0.0)
    assert not p.counts.any()
    # an empty list: the decomposition ran, nothing is in front
    p = unchanged(k0[:0], k1[:0], m[:0], f, CAMS, lambda s: s[0] == 1.0 and abs(float(s[1]) - 1.0) < 1e-6)
    assert not p.counts.any()
    # a NaN passes nothing
    bad = k0.copy()
    bad["x"] = np.nan
    p = unchanged(bad, k1, m, f, CAMS, lambda s: s[0] == 1.0)
    assert not p.counts.any()


# ---- filtering ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(257, 1), (257, 2), (257, 3), (1000, 4)])
def test_filter_is_the_numpy_subset_in_order(amd, n, seed):
    """0.7 px of noise and 20 % outliers under the true F: the kept list is the numpy statement's subset, in order.  Outliers that
    happen to triangulate in front stay; that is the statement."""
    k0, k1, m, sc = scene_case(amd, seed, n, sigma=0.7, outliers=0.2)
    rng = np.random.default_rng(seed)
    m = m[rng.permutation(n)]  # (list order is not keypoint order)
    f = sc["f"].astype(np.float32)
    kept, pose, pts = amd.recover_pose_host(k0, k1, m, f, *CAMS, points=True)
    ref = reference(amd, k0, k1, m, f, pose)
    assert pose.found == 1 and [int(v) for v in pose.counts] == [int(v) for v in ref["in_front"]] and pose.winner == ref["winner"]
    assert np.array_equal(kept, m[ref["keep"]]) and len(kept) == pose.counts[pose.winner]
    print("kept", len(kept), "of", n, "outliers", int(sc["out"].sum()))
    assert n - int(sc["out"].sum()) <= len(kept) < n  # every true inlier is in front; some outlier is not
    assert pts.shape == (len(kept), 3)
    # (the points of displaced matches are ill-conditioned: compared where the scene is true)
    true = ~sc["out"][m["index_0"]][ref["keep"]]
    assert np.abs(pts[true] - ref["points"][true]).max() <= 4.0e-4


def test_points_is_optional_and_changes_nothing(amd):
    k0, k1, m, sc = scene_case(amd, 9, 65, sigma=0.7, outliers=0.2)
    f = sc["f"].astype(np.float32)
    a, pa = amd.recover_pose_host(k0, k1, m, f, *CAMS)
    b, pb, _ = amd.recover_pose_host(k0, k1, m, f, *CAMS, points=True)
    assert np.array_equal(a, b) and bytes(pa) == bytes(pb)
