"""Absolute pose by the seeded 6-point resection RANSAC on the host (akz_estimate_resection, akz_refine_resection,
akz_resection_seeded_host; no GPU call): the surface and the refusals, the sampler and the stopping count at K = 6 against the
Python restatement of tests/test_seeded_ransac_host.py, the trial model against an independent numpy statement
(tests/resection_numpy.py), quality as a condition on noise-free scenes, the bookkeeping of rounds, winner and stop, the join
helper, and three views end to end."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_numpy as pn
import resection_numpy as rn
from test_homography_host import _ident_matches, _kp
from test_match_pairs_host import ROOT, _status
from test_seeded_ransac_host import M64, py_need, py_sample

NEW_SYMBOLS = ("akz_estimate_resection", "akz_refine_resection", "akz_resection_seeded_host", "akz_resection_seeded_problems")
K = 6
# The largest disagreement with the numpy statement over the 200 samples of test_trial_model_equals_numpy, measured on this
# code: 1.6e-7 rad and 2.1e-6 of |t| (the f32 rounding of the result alone is 6e-8).  The bound is ten times that: the library
# decomposes A^T A, whose condition number is the square of what numpy's SVD of A sees, and six points leave little to spare.
ANGLE_MEASURED, T_MEASURED = 1.6e-7, 2.1e-6
ANGLE_BOUND, T_BOUND = 10 * ANGLE_MEASURED, 10 * T_MEASURED


def options(amd, **kw):
    kw.setdefault("epsilon_inliers", 1.0)
    return amd.RansacOptions(model_kind=amd.RANSAC_RESECTION, **kw)


def f32_inliers(pose, points, pixels, camera, eps):
    """the inlier rule of include/akaze_hip.h restated in numpy float32 (element-wise IEEE operations in the written order)"""
    f = np.float32
    r, t = pose.R.astype(f), pose.T.astype(f)
    X, Y, Z = (points[:, k].astype(f) for k in range(3))
    u, v = pixels[:, 0].astype(f), pixels[:, 1].astype(f)
    fx, fy, cx, cy = (f(c) for c in camera)
    c = [((r[k, 0] * X + r[k, 1] * Y) + r[k, 2] * Z) + t[k] for k in range(3)]
    ex = fx * c[0] - (u - cx) * c[2]
    ey = fy * c[1] - (v - cy) * c[2]
    return (c[2] > 0) & (ex * ex + ey * ey < (f(eps) * f(eps)) * (c[2] * c[2]))


# ---- the surface -------------------------------------------------------------------------------------------------------------
def test_symbols_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"#define\s+AKZ_RANSAC_RESECTION\s+4\b", hdr) and amd.RANSAC_RESECTION == 4
    assert "typedef struct akz_resection_problem" in hdr and "typedef struct akz_resection {" in hdr
    assert C.sizeof(amd.Resection) == 64 and C.sizeof(amd.ResectionProblem) == 56 and C.sizeof(amd.RansacOptions) == 80
    assert len(amd.Resection().words()) == 16
    for name in ("Resection", "estimate_resection", "refine_resection", "resection_seeded_host", "correspondences_2d3d"):
        assert callable(getattr(amd, name)), name
    assert callable(amd.Context.resection_seeded)


def test_refusals(amd):
    L, bad = amd.lib(), _status(amd)
    sc = rn.make_scene(1, 40, 10)
    pts, pix = sc["points"], sc["pixels"]
    fp = C.POINTER(C.c_float)
    cam = amd.Camera(*sc["camera"])
    kept = np.full(50, 0xA5A5A5A5, np.uint32)
    n, it, run = C.c_uint64(12345), C.c_uint32(99), C.c_uint64(77)
    pose = amd.Resection()
    C.memset(C.byref(pose), 0x5A, C.sizeof(pose))
    good = options(amd, max_trials=128)

    def problem(points=pts.ctypes.data_as(fp), pixels=pix.ctypes.data_as(fp), count=50, camera=cam):
        return amd.ResectionProblem(points, pixels, count, camera)

    def seeded(opt=good, prob=problem(), keptp=kept.ctypes.data, np_=C.byref(n), posep=C.byref(pose)):
        return L.akz_resection_seeded_host(C.byref(prob) if prob is not None else None, C.byref(opt) if opt is not None else None, 0, keptp,
                                           np_, posep, C.byref(it), C.byref(run))
    # the options: the family's list with 4 as the one kind, and guided
    assert seeded(opt=None) == bad
    assert seeded(opt=good.copy(struct_size=C.sizeof(good) - 8)) == bad and seeded(opt=good.copy(struct_size=0)) == bad
    for kind in (0, 1, 2, 3, 5, -1):
        assert seeded(opt=good.copy(model_kind=kind)) == bad, kind
    assert seeded(opt=good.copy(max_trials=(1 << 24) + 1)) == bad
    for conf in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert seeded(opt=good.copy(confidence=conf)) == bad, conf
    assert seeded(opt=good.copy(guided=1)) == bad
    for eps in (0.0, -1.0, float("nan"), float("inf")):                  # the refit's refusal, with a refit only
        assert seeded(opt=good.copy(refine_iterations=2, epsilon_inliers=eps)) == bad, eps
    # the problem
    assert seeded(prob=None) == bad and seeded(np_=None) == bad and seeded(posep=None) == bad and seeded(keptp=None) == bad
    assert seeded(prob=problem(points=None)) == bad and seeded(prob=problem(pixels=None)) == bad
    assert seeded(prob=problem(count=1 << 32)) == bad and seeded(prob=problem(count=M64)) == bad
    bad_cams = [amd.Camera(0.0, 1400.0, 960.0, 540.0), amd.Camera(1400.0, 0.0, 960.0, 540.0)]
    for field in ("fx", "fy", "cx", "cy"):
        for v in (float("nan"), float("inf"), float("-inf")):
            c = amd.Camera(*sc["camera"])
            setattr(c, field, v)
            bad_cams.append(c)
    for c in bad_cams:
        assert seeded(prob=problem(camera=c)) == bad, (c.fx, c.fy, c.cx, c.cy)
    # the refit alone
    ident = amd.Resection()
    ident.r[0] = ident.r[4] = ident.r[8] = 1.0

    def refine(prob=problem(), pin=C.byref(ident), eps=1.0, keptp=kept.ctypes.data, np_=C.byref(n)):
        return L.akz_refine_resection(C.byref(prob) if prob is not None else None, pin, eps, 2, keptp, np_, C.byref(pose), C.byref(it))
    assert refine(prob=None) == bad and refine(pin=None) == bad and refine(np_=None) == bad and refine(keptp=None) == bad
    assert refine(prob=problem(points=None)) == bad and refine(prob=problem(count=1 << 32)) == bad
    assert refine(prob=problem(camera=bad_cams[0])) == bad
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert refine(eps=eps) == bad, eps
    # the sample
    found = C.c_int(55)
    est = L.akz_estimate_resection
    assert est(None, pix.ctypes.data_as(fp), C.byref(cam), C.byref(pose), C.byref(found)) == bad
    assert est(pts.ctypes.data_as(fp), None, C.byref(cam), C.byref(pose), C.byref(found)) == bad
    assert est(pts.ctypes.data_as(fp), pix.ctypes.data_as(fp), None, C.byref(pose), C.byref(found)) == bad
    assert est(pts.ctypes.data_as(fp), pix.ctypes.data_as(fp), C.byref(cam), None, C.byref(found)) == bad
    assert est(pts.ctypes.data_as(fp), pix.ctypes.data_as(fp), C.byref(bad_cams[1]), C.byref(pose), C.byref(found)) == bad
    # nothing was written by a refused call
    assert n.value == 12345 and it.value == 99 and run.value == 77 and found.value == 55
    assert bytes(pose) == b"\x5a" * 64 and np.all(kept == 0xA5A5A5A5)
    # every other call keeps refusing the new kind
    k0 = _kp(amd, pix)
    with pytest.raises(amd.AkazeError):
        amd.remove_outliers_seeded(k0, k0, _ident_matches(amd, 50), options(amd))
    # accepted: an epsilon the refit would refuse without a refit; an empty problem with NULL arrays; the trailing pointers NULL
    assert seeded(opt=good.copy(epsilon_inliers=float("inf"))) == 0
    assert seeded(prob=problem(points=None, pixels=None, count=0), keptp=None) == 0 and n.value == 0 and pose.found == 0 and run.value == 0
    assert L.akz_resection_seeded_host(C.byref(problem()), C.byref(good), 0, kept.ctypes.data, C.byref(n), C.byref(pose), None, None) == 0
    assert n.value <= 50


# ---- the sampler and the stopping rule at K = 6 ------------------------------------------------------------------------------
def test_sample_of_six(amd):
    for n in (6, 7, 9, 64, 1000, (1 << 32) - 1):
        for s0, s1, stream in ((42, 69, 0), (0, 0, 0), (M64, M64, M64), (7, 1 << 63, 12345), (42, 69, 1)):
            for trial in (0, 1, 2, 127, 128, 999, (1 << 24) - 1):
                got = amd.draw_sample_seeded(s0, s1, stream, trial, n, K)
                assert got.tolist() == py_sample(s0, s1, stream, trial, n, K), (n, s0, s1, stream, trial)
                assert len(got) == K and np.all(np.diff(got.astype(np.int64)) > 0) and int(got[-1]) < n   # distinct, ascending, below n
    a = [amd.draw_sample_seeded(42, 69, 0, t, 1000, K).tolist() for t in range(16)]
    b = [amd.draw_sample_seeded(42, 69, 1, t, 1000, K).tolist() for t in range(16)]
    assert all(x != y for x, y in zip(a, b))
    assert a == [amd.draw_sample_seeded(42, 69, 0, t, 1000, K).tolist() for t in range(16)]
    # 5 stays refused, and too few elements
    out = np.full(8, 99, np.uint64)
    po = out.ctypes.data_as(C.POINTER(C.c_uint64))
    L, bad = amd.lib(), _status(amd)
    assert L.akz_draw_sample_seeded(1, 2, 0, 0, 100, 5, po) == bad and L.akz_draw_sample_seeded(1, 2, 0, 0, 5, 6, po) == bad
    assert np.all(out == 99)


def test_sample_of_six_is_uniform(amd):
    """20 000 trials at n = 16, K = 6: an index is in a sample with probability 3 / 8, so its count is binomial with mean 7 500 and
    standard deviation sqrt(20000 * 3/8 * 5/8) = 68.5; every index within 6 of them, the bound of the test for K = 4 and 8."""
    trials, n = 20000, 16
    count = np.zeros(n, np.int64)
    for t in range(trials):
        count[amd.draw_sample_seeded(42, 69, 3, t, n, K).astype(np.int64)] += 1
    assert count.sum() == trials * K
    sd = (trials * (K / n) * (1 - K / n)) ** 0.5
    assert np.all(np.abs(count - trials * K / n) <= 6 * sd), count


def test_required_inliers_of_six(amd):
    for n in (6, 9, 64, 257, 1000):
        for conf in (0.5, 0.99, 0.999999):
            prev = n
            for trials in (1, 2, 127, 128, 129, 256, 1000, 1024, 2177, 1 << 24):
                need = amd.ransac_required_inliers(n, K, trials, conf)
                assert need == py_need(n, K, trials, conf), (n, conf, trials)
                assert 1 <= need <= prev <= n, (n, conf, trials)
                prev = need


# ---- the trial model ---------------------------------------------------------------------------------------------------------
def test_trial_model_equals_numpy(amd):
    sc = rn.make_scene(1000, 400, 0)
    rng = np.random.default_rng(5)
    worst_a = worst_t = 0.0
    for _ in range(200):
        idx = np.sort(rng.choice(400, 6, replace=False))
        pose = amd.estimate_resection(sc["points"][idx], sc["pixels"][idx], sc["camera"])
        ref = rn.dlt(sc["points"][idx], sc["pixels"][idx])
        assert pose.found == 1 and ref is not None, idx
        ea, et = rn.pose_error(pose.R, pose.T, ref[0], ref[1])
        worst_a, worst_t = max(worst_a, ea), max(worst_t, et)
        assert abs(np.linalg.det(pose.R.astype(np.float64)) - 1.0) < 1e-5 and pose.singular_values[0] == 1.0
        assert np.allclose(pose.singular_values, ref[2], atol=1e-5)
    print(f"largest disagreement with numpy over 200 samples: {worst_a:.3e} rad, {worst_t:.3e} of |t|")
    assert worst_a <= ANGLE_BOUND and worst_t <= T_BOUND, (worst_a, worst_t)


def test_samples_without_a_model(amd):
    sc = rn.make_scene(7, 6, 0)
    xc = sc["points"].astype(np.float64) @ sc["R"].T + sc["t"]
    xc[:, 2] = 5.0                                                    # six points of the plane z = 5 in front of the camera
    flat = ((xc - sc["t"]) @ sc["R"]).astype(np.float32)
    pose = amd.estimate_resection(flat, rn.project(sc["R"], sc["t"], flat)[0].astype(np.float32), sc["camera"])
    assert pose.found == 0 and not pose.words().any()
    pts, pix = sc["points"].copy(), sc["pixels"].copy()
    assert amd.estimate_resection(pts, pix, sc["camera"]).found == 1
    pts[3], pix[3] = pts[2], pix[2]                                   # a repeated correspondence: five points
    assert amd.estimate_resection(pts, pix, sc["camera"]).found == 0


def test_a_sample_is_one_fit_of_the_refit(amd):
    """fit(S) is one function: the model of six correspondences equals one accepted fit of refine_resection over those six (from a
    pose that keeps all of them), bit for bit"""
    ident = amd.Resection()
    ident.r[0] = ident.r[4] = ident.r[8] = 1.0
    for seed in range(8):
        sc = rn.make_scene(50 + seed, 6, 0)
        kept, pose, its = amd.refine_resection(sc["points"], sc["pixels"], sc["camera"], ident, 1e9, 1)
        assert len(kept) == 6 and its == 1
        assert np.array_equal(pose.words(), amd.estimate_resection(sc["points"], sc["pixels"], sc["camera"]).words()), seed


# ---- quality, as a condition ---------------------------------------------------------------------------------------------------
def test_quality_on_noise_free_scenes(amd):
    """24 scenes of 200 true correspondences and 50 outliers, eps 1 px, 128 trials, two refit iterations: found, and the kept set
    is exactly the true one"""
    for s in range(24):
        sc = rn.make_scene(100 + s)
        opt = options(amd, max_trials=128, confidence=0.0, refine_iterations=2)
        kept, pose, its, run = amd.resection_seeded_host(sc["points"], sc["pixels"], sc["camera"], opt, stream=s)
        assert pose.found == 1 and run == 128, s
        assert np.array_equal(kept, np.flatnonzero(sc["true"])), (s, len(kept))
        ea, et = rn.pose_error(pose.R, pose.T, sc["R"], sc["t"])
        assert ea < 1e-4 and et < 1e-3, (s, ea, et)


# ---- bookkeeping ---------------------------------------------------------------------------------------------------------------
def test_rounds_and_reproducibility(amd):
    sc = rn.make_scene(11, 60, 15)
    args = (sc["points"], sc["pixels"], sc["camera"])
    for max_trials in (0, 1, 127, 128, 129, 300):
        opt = options(amd, max_trials=max_trials, confidence=0.0)
        kept, pose, its, run = amd.resection_seeded_host(*args, opt, stream=5)
        again = amd.resection_seeded_host(*args, opt, stream=5)
        assert np.array_equal(kept, again[0]) and np.array_equal(pose.words(), again[1].words()) and again[2:] == (its, run)
        assert run == max_trials and its == 0                      # confidence 0: exactly max_trials
        if pose.found:                                             # the kept list is the problem filtered by the returned pose
            assert np.array_equal(kept, np.flatnonzero(f32_inliers(pose, sc["points"], sc["pixels"], sc["camera"], 1.0))), max_trials
        else:
            assert len(kept) == 0 and not pose.words().any()
        if max_trials == 0:
            assert pose.found == 0
        for conf in (0.5, 0.99):                                   # with the rule on: whole rounds, and never past max_trials
            run_c = amd.resection_seeded_host(*args, opt.copy(confidence=conf), stream=5)[3]
            assert run_c <= max_trials and (run_c == max_trials or run_c % amd.RANSAC_ROUND == 0), (max_trials, conf, run_c)
    opt = options(amd, max_trials=16, confidence=0.0)   # another stream draws other samples
    a, b = (amd.resection_seeded_host(*args, opt, stream=s)[1] for s in (0, 1))
    assert a.found and b.found and not np.array_equal(a.words(), b.words())
    # fewer than K correspondences: nothing run
    kept, pose, its, run = amd.resection_seeded_host(sc["points"][:5], sc["pixels"][:5], sc["camera"], options(amd, refine_iterations=2))
    assert len(kept) == 0 and pose.found == 0 and not pose.words().any() and (its, run) == (0, 0)


def test_the_winner_is_the_first_maximum(amd):
    sc = rn.make_scene(12, 40, 40)
    pts, pix, cam = sc["points"], sc["pixels"], sc["camera"]
    opt = options(amd, max_trials=200, confidence=0.0, seed=(3, 4))
    kept, pose, _, run = amd.resection_seeded_host(pts, pix, cam, opt, stream=9)
    best, winner = 0, None
    for t in range(200):
        idx = amd.draw_sample_seeded(3, 4, 9, t, len(pts), K).astype(np.int64)
        model = amd.estimate_resection(pts[idx], pix[idx], cam)
        if not model.found:
            continue
        count = int(f32_inliers(model, pts, pix, cam, 1.0).sum())
        if count > best:
            best, winner = count, model
    assert winner is not None and pose.found == 1 and run == 200
    assert np.array_equal(pose.words(), winner.words()) and len(kept) == best


def test_both_stopping_branches(amd):
    """98 true of 200, noise-free, confidence 0.99: need(200, 6, T) is 115, 103, 96 after one, two, three rounds, so the problem
    stops after the third round -- the first in which best >= need -- and not before; 60 of 200 never reaches its count in two
    rounds and runs to max_trials with the rule on"""
    assert [amd.ransac_required_inliers(200, K, T, 0.99) for T in (128, 256, 384)] == [115, 103, 96]
    sc = rn.make_scene(13, 98, 102)
    opt = options(amd, max_trials=1000, confidence=0.99)
    kept, pose, _, run = amd.resection_seeded_host(sc["points"], sc["pixels"], sc["camera"], opt, stream=2)
    assert pose.found == 1 and run == 3 * amd.RANSAC_ROUND < 1000, run
    assert len(kept) >= amd.ransac_required_inliers(200, K, run, 0.99)
    assert len(kept) < amd.ransac_required_inliers(200, K, run - amd.RANSAC_ROUND, 0.99)   # (the count can only have grown since)
    sc = rn.make_scene(14, 60, 140)
    opt = options(amd, max_trials=256, confidence=0.99)
    kept, pose, _, run = amd.resection_seeded_host(sc["points"], sc["pixels"], sc["camera"], opt, stream=2)
    assert pose.found == 1 and run == 256 and len(kept) < amd.ransac_required_inliers(200, K, run, 0.99)


def test_refit_is_refine_on_the_unrefined_result(amd):
    sc = rn.make_scene(15, 200, 50, noise=0.5)
    args = (sc["points"], sc["pixels"], sc["camera"])
    for conf in (0.0, 0.99):
        plain = amd.resection_seeded_host(*args, options(amd, epsilon_inliers=3.0, confidence=conf), stream=2)
        assert plain[1].found == 1
        for its in (1, 2, 8):
            got = amd.resection_seeded_host(*args, options(amd, epsilon_inliers=3.0, confidence=conf, refine_iterations=its), stream=2)
            exp = amd.refine_resection(*args, plain[1], 3.0, its)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1].words(), exp[1].words()) and got[2] == exp[2] and got[3] == plain[3]
            assert len(got[0]) >= len(plain[0])


# ---- the join helper -----------------------------------------------------------------------------------------------------------
def test_correspondences_2d3d(amd):
    ab = np.zeros(4, amd.MATCH_DTYPE)
    ab["index_0"], ab["index_1"] = [7, 3, 7, 9], [0, 1, 2, 3]           # A's keypoint 7 occurs twice: record 0 is the first
    points_ab = np.arange(12, dtype=np.float32).reshape(4, 3)
    ac = np.zeros(5, amd.MATCH_DTYPE)
    ac["index_0"], ac["index_1"] = [9, 5, 7, 3, 7], [4, 0, 2, 1, 3]     # 5 is unmatched in (A, B); 7 occurs twice here too
    kc = _kp(amd, np.array([[10, 11], [20, 21], [30, 31], [40, 41], [50, 51]], np.float32))
    pts, pix, at_ab, at_ac = amd.correspondences_2d3d(ab, points_ab, ac, kc)
    assert at_ac.tolist() == [0, 2, 3, 4] and at_ab.tolist() == [3, 0, 1, 0]
    assert pts.dtype == np.float32 and np.array_equal(pts, points_ab[[3, 0, 1, 0]])
    assert pix.dtype == np.float32 and pix.tolist() == [[50, 51], [30, 31], [20, 21], [40, 41]]
    e = amd.correspondences_2d3d(ab[:0], points_ab[:0], ac, kc)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 2) and len(e[2]) == len(e[3]) == 0


# ---- three views end to end, on the host ---------------------------------------------------------------------------------------
def test_three_views_on_the_host(amd):
    """views A and B give recover_pose_host's points (at |t_AB| = 1, in A's frame); a synthetic (A, C) list joins them with C's
    pixels; the resection places C: every true correspondence is kept at 1 px and the pose is C's, at that scale"""
    cams = ((1180.0, 1230.0, 940.0, 560.0), (1250.0, 1190.0, 985.0, 520.0))
    cam_c = (1300.0, 1310.0, 950.0, 530.0)
    n = 120
    sc = pn.pose_scene(77, n, cams=cams)
    ka, kb = _kp(amd, sc["p0"].astype(np.float32)), _kp(amd, sc["q1"].astype(np.float32))
    kept_ab, pose_ab, pts_ab = amd.recover_pose_host(ka, kb, _ident_matches(amd, n), sc["f"].astype(np.float32), *cams, points=True)
    assert pose_ab.found == 1 and len(kept_ab) == n
    # C: a camera 0.3 |t_AB| to the side of A, turned a little
    scale = np.linalg.norm(sc["t"])
    r_c = rn.rodrigues(np.array([0.02, -0.05, 0.03]))
    t_c = np.array([-0.3, 0.1, 0.05]) * scale
    pix_c, z = rn.project(r_c, t_c, sc["x"], cam_c)
    assert np.all(z > 0)
    rng = np.random.default_rng(3)
    seen = np.sort(rng.choice(n, 80, replace=False))                   # C sees 80 of A's keypoints ...
    kc = np.zeros(100, amd.KEYPOINT_DTYPE)
    kc["x"][:80], kc["y"][:80] = pix_c[seen, 0], pix_c[seen, 1]
    kc["x"][80:], kc["y"][80:] = rng.uniform(0, 1920, 20), rng.uniform(0, 1080, 20)
    ac = np.zeros(100, amd.MATCH_DTYPE)
    ac["index_0"][:80], ac["index_1"][:80] = seen, np.arange(80)
    ac["index_0"][80:], ac["index_1"][80:] = rng.choice(n, 20), np.arange(80, 100)   # ... and 20 wrong matches
    ac = ac[rng.permutation(100)]
    pts, pix, at_ab, at_ac = amd.correspondences_2d3d(kept_ab, pts_ab, ac, kc)
    assert len(pts) == 100
    true = ac["index_1"][at_ac] < 80
    opt = options(amd, max_trials=256, confidence=0.0, refine_iterations=2)
    kept, pose, its, run = amd.resection_seeded_host(pts, pix, cam_c, opt)
    assert pose.found == 1 and set(np.flatnonzero(true)) <= set(kept.tolist()), (len(kept), int(true.sum()))
    ea, et = rn.pose_error(pose.R, pose.T, r_c, t_c / scale)
    assert ea < 1e-3 and et < 1e-2, (ea, et)
