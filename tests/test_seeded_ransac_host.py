"""The seeded RANSAC on the host (akz_draw_sample_seeded, akz_ransac_required_inliers, akz_remove_outliers_seeded; no GPU call):
declarations, the sample and the stopping count against an independent restatement in Python integers and floats, the host
statement's promises (reproducible, the thread's random source untouched, rounds of 128, the filter by the returned model, the
refit as refine_* on the unrefined result), the two stopping branches on planted scenes, and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_fundamental_refit_host import error_rule
from test_gpu_fundamental_refit import planted_case as planted_f
from test_gpu_homography import inlier_rule
from test_gpu_homography_refit import planted_case as planted_h
from test_match_pairs_host import ROOT, _color, _status

NEW_SYMBOLS = ("akz_ransac_options_default", "akz_draw_sample_seeded", "akz_ransac_required_inliers", "akz_remove_outliers_seeded",
               "akz_match_features_seeded_pairs")
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
EPS = {"F": 0.02, "H": 3.0}   # the epsilons of the two refit test files, on the same scenes
KIND = {"H": 0, "F": 1}       # AKZ_GUIDED_HOMOGRAPHY, AKZ_GUIDED_FUNDAMENTAL
K = {"H": 4, "F": 8}
# The two stopping branches that tests/test_gpu_seeded_ransac.py relies on, chosen here from the host statement: (model, matches,
# scene seed, options, stream).  The trial model of the fundamental matrix is the reference's -- the right vector of the smallest
# of EIGHT singular values, in raw pixel coordinates -- and at the refit tests' epsilon 0.02 its winner keeps about 8 of 257
# matches: FULL runs to max_trials with the rule on.  At epsilon 4 the same scene's winners keep about half, and stream 4 reaches
# need(257, 8, 384, 0.99) in its third round: EARLY.  The homography reaches its count in the first round: EARLY_H.
EARLY = ("F", 257, 757, dict(max_trials=1025, confidence=0.99, epsilon_inliers=4.0), 4)
EARLY_H = ("H", 257, 757, dict(max_trials=1000, confidence=0.99), 0)
FULL = ("F", 257, 757, dict(max_trials=1000, confidence=0.99), 0)


# ---- the statement of include/akaze_hip.h in Python integers and floats -------------------------------------------------------
def mix64(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_sample(seed0, seed1, stream, trial, n, k):
    k0 = mix64((seed0 + G) & M64)
    k1 = mix64(seed1 ^ k0)
    ks = mix64((k1 + G * (stream + 1)) & M64)
    picked = set()
    for i in range(k):
        j = n - k + i
        v = mix64((ks + G * (8 * trial + i + 1)) & M64)
        r = (v * (j + 1)) >> 64
        picked.add(j if r in picked else r)
    return sorted(picked)


def py_enough(b, n, k, trials, confidence):
    w = float(b) / float(n)
    wk = w
    for _ in range(k - 1):
        wk = wk * w
    q, res, t = 1.0 - wk, 1.0, trials
    while t:
        if t & 1:
            res = res * q
        t >>= 1
        if t:
            q = q * q
    return res <= 1.0 - confidence


def py_need(n, k, trials, confidence):
    return next(b for b in range(1, n + 1) if py_enough(b, n, k, trials, confidence))


# ---- planted scenes: the raw list that descriptor_match returns for them, without a GPU -----------------------------------------
def planted(amd, model, n, seed):
    """-> (fa, fb, raw): planted_case of the model's GPU refit tests and its planted matches in list order"""
    fa, fb = (planted_f(amd, n, seed) if model == "F" else planted_h(amd, n, seed)[:2])
    where = {d.tobytes(): j for j, d in enumerate(fb[1])}
    raw = np.zeros(n, amd.MATCH_DTYPE)
    raw["index_0"] = np.arange(n)
    raw["index_1"] = [where[d.tobytes()] for d in fa[1]]
    return fa, fb, raw


def options(amd, model, **kw):
    kw.setdefault("epsilon_inliers", EPS[model])
    return amd.RansacOptions(model_kind=KIND[model], **kw)


def rule(model, f, k0, k1, raw, eps):
    return (error_rule if model == "F" else inlier_rule)(f, k0, k1, raw, eps)


def same4(got, exp, what=None):
    (gm, gf, gi, gt), (em, ef, ei, et) = got, exp
    assert gm.dtype == em.dtype and np.array_equal(gm, em), (what, len(gm), len(em))
    assert (gf is None) == (ef is None), what
    if gf is not None:
        assert np.array_equal(np.asarray(gf, np.float32).view(np.uint32), np.asarray(ef, np.float32).view(np.uint32)), (what, gf, ef)
    assert (gi, gt) == (ei, et), (what, gi, ei, gt, et)


# ---- declarations ----------------------------------------------------------------------------------------------------------
def test_symbols_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", hdr), name
    assert L.akz_abi_version() == 6
    assert "typedef struct akz_ransac_options" in hdr
    for name in ("RansacOptions", "draw_sample_seeded", "ransac_required_inliers", "remove_outliers_seeded", "match_features_seeded",
                 "match_features_seeded_pairs"):
        assert callable(getattr(amd, name)), name
    assert callable(amd.Context.match_features_seeded_pairs)
    o = amd.RansacOptions()
    assert (o.struct_size, o.model_kind, o.lowes_ratio, o.max_trials, o.refine_iterations, o.confidence, list(o.seed), o.stream_base,
            o.guided) == (C.sizeof(o), amd.GUIDED_FUNDAMENTAL, 0.86, 1000, 0, 0.99, [42, 69], 0, 0)
    assert o.epsilon_inliers == np.float32(0.02)


# ---- the sample --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 8])
def test_sample_equals_the_python_restatement(amd, k):
    for n in (k, k + 1, 9, 64, 1000, (1 << 32) - 1):
        for s0, s1, stream in ((42, 69, 0), (0, 0, 0), (M64, M64, M64), (7, 1 << 63, 12345), (42, 69, 1)):
            for trial in (0, 1, 2, 127, 128, 999, (1 << 24) - 1):
                got = amd.draw_sample_seeded(s0, s1, stream, trial, n, k)
                assert got.tolist() == py_sample(s0, s1, stream, trial, n, k), (n, s0, s1, stream, trial)
                assert len(got) == k and np.all(np.diff(got.astype(np.int64)) > 0) and int(got[-1]) < n   # distinct, ascending, below n


def test_streams_give_different_sequences(amd):
    a = [amd.draw_sample_seeded(42, 69, 0, t, 1000, 8).tolist() for t in range(16)]
    b = [amd.draw_sample_seeded(42, 69, 1, t, 1000, 8).tolist() for t in range(16)]
    c = [amd.draw_sample_seeded(42, 70, 0, t, 1000, 8).tolist() for t in range(16)]
    assert all(x != y for x, y in zip(a, b)) and all(x != y for x, y in zip(a, c))
    assert a == [amd.draw_sample_seeded(42, 69, 0, t, 1000, 8).tolist() for t in range(16)]


def test_sample_is_uniform(amd):
    """20 000 trials at n = 16, K = 4: an index is in a sample with probability K / n = 1 / 4, so its count is binomial with
    mean 5 000 and standard deviation sqrt(20000 * 1/4 * 3/4) = 61.2; every index within 6 of them (a fair generator fails this
    about once in 10^8 runs of 16 indices)."""
    trials, n, k = 20000, 16, 4
    count = np.zeros(n, np.int64)
    for t in range(trials):
        count[amd.draw_sample_seeded(42, 69, 3, t, n, k).astype(np.int64)] += 1
    assert count.sum() == trials * k
    sd = (trials * (k / n) * (1 - k / n)) ** 0.5
    assert np.all(np.abs(count - trials * k / n) <= 6 * sd), count


# ---- need --------------------------------------------------------------------------------------------------------------------
def test_required_inliers_equal_the_python_restatement(amd):
    for k in (4, 8):
        for n in (k, 9, 64, 257, 1000):
            for conf in (0.5, 0.99, 0.999999):
                prev = n
                for trials in (1, 2, 127, 128, 129, 256, 1000, 1024, 2177, 1 << 24):
                    need = amd.ransac_required_inliers(n, k, trials, conf)
                    assert need == py_need(n, k, trials, conf), (k, n, conf, trials)
                    assert 1 <= need <= prev <= n, (k, n, conf, trials)      # at most n, nonincreasing in trials
                    prev = need
    assert amd.ransac_required_inliers(1000, 8, 1, 0.999999) == 1000
    assert amd.ransac_required_inliers(1 << 40, 8, 1000, 0.99) <= 1 << 40


def test_required_inliers_refusals(amd):
    L, bad = amd.lib(), _status(amd)
    need = C.c_uint64(77)
    for args in ((1000, 5, 10, 0.99), (0, 8, 10, 0.99), (1000, 8, 0, 0.99), (1000, 8, 10, 0.0), (1000, 8, 10, 1.0), (1000, 8, 10, -0.5),
                 (1000, 8, 10, float("nan"))):
        assert L.akz_ransac_required_inliers(args[0], args[1], args[2], args[3], C.byref(need)) == bad, args
    assert L.akz_ransac_required_inliers(1000, 8, 10, 0.99, None) == bad
    assert need.value == 77
    out = np.full(8, 99, np.uint64)
    po = out.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.akz_draw_sample_seeded(1, 2, 0, 0, 7, 8, po) == bad and L.akz_draw_sample_seeded(1, 2, 0, 0, 100, 5, po) == bad
    assert L.akz_draw_sample_seeded(1, 2, 0, 0, 100, 8, None) == bad and np.all(out == 99)


# ---- the host statement ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(amd):
    """the planted scenes this file uses (built once, left unchanged)"""
    want = {("F", 7, 507), ("F", 8, 508), ("F", 9, 509), ("F", 65, 575), ("F", 257, 757), ("H", 3, 503), ("H", 4, 504), ("H", 5, 505),
            ("H", 65, 565), ("H", 257, 757)}
    return {key: planted(amd, *key) for key in want}


@pytest.mark.parametrize("model,n,seed", [("F", 9, 509), ("F", 65, 575), ("F", 257, 757), ("H", 5, 505), ("H", 65, 565), ("H", 257, 757)])
def test_rounds_filter_and_reproducibility(amd, scenes, model, n, seed):
    fa, fb, raw = scenes[(model, n, seed)]
    amd.random_seed(42, 69)
    fresh = _color(amd)
    amd.random_seed(42, 69)
    for max_trials in (0, 1, 127, 128, 129, 300):
        opt = options(amd, model, max_trials=max_trials, confidence=0.0)
        got = amd.remove_outliers_seeded(fa[0], fb[0], raw, opt, stream=5)
        same4(amd.remove_outliers_seeded(fa[0], fb[0], raw, opt, stream=5), got, "again")
        kept, f, its, run = got
        assert run == max_trials and its == 0                     # confidence 0: exactly max_trials
        if f is not None:                                         # the kept list is the raw list filtered by the returned model
            assert np.array_equal(kept, raw[rule(model, f, fa[0], fb[0], raw, EPS[model])]), max_trials
        elif model == "H" or max_trials == 0:
            assert np.array_equal(kept, raw)                      # (no winner -- H: every match; F: the zero model's error is 0)
        if max_trials == 0:
            assert f is None
        for conf in (0.5, 0.99):                                  # with the rule on: whole rounds, and never past max_trials
            run_c = amd.remove_outliers_seeded(fa[0], fb[0], raw, opt.copy(confidence=conf), stream=5)[3]
            assert run_c <= max_trials and (run_c == max_trials or run_c % amd.RANSAC_ROUND == 0), (max_trials, conf, run_c)
    # another stream draws other samples on the same list
    opt = options(amd, model, max_trials=128, confidence=0.0)
    if n > 9:
        a, b = (amd.remove_outliers_seeded(fa[0], fb[0], raw, opt, stream=s)[1] for s in (0, 1))
        assert a is not None and b is not None and not np.array_equal(a, b)
    amd.random_seed(42, 69)
    assert _color(amd) == fresh
    # the thread's source: not read, not advanced
    amd.random_seed(11, 12)
    before = _color(amd)
    amd.random_seed(11, 12)
    amd.remove_outliers_seeded(fa[0], fb[0], raw, options(amd, model, max_trials=300, refine_iterations=2), stream=1)
    assert _color(amd) == before


@pytest.mark.parametrize("model,n,seed", [("F", 7, 507), ("H", 3, 503)])
def test_fewer_than_k_matches(amd, scenes, model, n, seed):
    fa, fb, raw = scenes[(model, n, seed)]
    kept, f, its, run = amd.remove_outliers_seeded(fa[0], fb[0], raw, options(amd, model, refine_iterations=2))
    assert np.array_equal(kept, raw) and f is None and its == 0 and run == 0
    e = np.zeros(0, amd.MATCH_DTYPE)
    kept, f, its, run = amd.remove_outliers_seeded(fa[0], fb[0], e, options(amd, model))
    assert len(kept) == 0 and f is None and run == 0


@pytest.mark.parametrize("model,n,seed", [("F", 8, 508), ("F", 257, 757), ("H", 4, 504), ("H", 257, 757)])
def test_refit_is_refine_on_the_unrefined_result(amd, scenes, model, n, seed):
    fa, fb, raw = scenes[(model, n, seed)]
    refine = amd.refine_fundamental_matrix if model == "F" else amd.refine_homography
    for conf in (0.0, 0.99):
        plain = amd.remove_outliers_seeded(fa[0], fb[0], raw, options(amd, model, confidence=conf), stream=2)
        for its in (1, 2, 8):
            got = amd.remove_outliers_seeded(fa[0], fb[0], raw, options(amd, model, confidence=conf, refine_iterations=its), stream=2)
            if plain[1] is None:
                same4(got, plain, (conf, its))
            else:
                same4(got, (*refine(fa[0], fb[0], raw, plain[1], EPS[model], its), plain[3]), (conf, its))


def test_both_stopping_branches(amd):
    """the cases the GPU test relies on: two stop before max_trials, one runs to max_trials with the rule on"""
    for (model, n, seed, kw, stream), rounds in ((EARLY, 3), (EARLY_H, 1)):
        fa, fb, raw = planted(amd, model, n, seed)
        kept, f, _, run = amd.remove_outliers_seeded(fa[0], fb[0], raw, options(amd, model, **kw), stream=stream)
        assert f is not None and run == rounds * amd.RANSAC_ROUND < kw["max_trials"], (model, run)
        assert len(kept) >= amd.ransac_required_inliers(n, K[model], run, kw["confidence"])
        if rounds > 1:   # (the round before did not reach its count: the winner's count can only have grown since)
            assert len(kept) < amd.ransac_required_inliers(n, K[model], run - amd.RANSAC_ROUND, kw["confidence"])
    model, n, seed, kw, stream = FULL
    fa, fb, raw = planted(amd, model, n, seed)
    kept, f, _, run = amd.remove_outliers_seeded(fa[0], fb[0], raw, options(amd, model, **kw), stream=stream)
    assert f is not None and run == kw["max_trials"] and len(kept) < amd.ransac_required_inliers(n, K[model], run, kw["confidence"])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(amd, scenes):
    L, bad = amd.lib(), _status(amd)
    fa, fb, raw = scenes[("F", 65, 575)]
    k0, k1 = fa[0], fb[0]
    out = np.zeros(len(raw), amd.MATCH_DTYPE)
    n = C.c_uint64(12345)
    f = np.full(9, 7.0, np.float32)
    found, it, run = C.c_int(55), C.c_uint32(99), C.c_uint64(77)
    good = options(amd, "F", max_trials=128)

    def call(opt=good, k0p=k0.ctypes.data, n0=len(k0), k1p=k1.ctypes.data, n1=len(k1), mp=raw.ctypes.data, outp=out.ctypes.data,
             np_=C.byref(n)):
        return L.akz_remove_outliers_seeded(k0p, n0, k1p, n1, mp, len(raw), C.byref(opt) if opt is not None else None, 0, outp, np_,
                                            f.ctypes.data_as(C.POINTER(C.c_float)), C.byref(found), C.byref(it), C.byref(run))
    amd.random_seed(42, 69)
    fresh = _color(amd)
    amd.random_seed(42, 69)
    assert call(opt=None) == bad
    assert call(opt=good.copy(struct_size=C.sizeof(good) - 8)) == bad and call(opt=good.copy(struct_size=0)) == bad
    assert call(opt=good.copy(model_kind=2)) == bad and call(opt=good.copy(model_kind=-1)) == bad
    assert call(opt=good.copy(max_trials=(1 << 24) + 1)) == bad
    for conf in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert call(opt=good.copy(confidence=conf)) == bad, conf
    for eps in (0.0, -1.0, float("nan"), float("inf")):                  # the refit's refusal, with a refit only
        assert call(opt=good.copy(refine_iterations=2, epsilon_inliers=eps)) == bad, eps
    assert call(np_=None) == bad and call(mp=None) == bad and call(outp=None) == bad
    assert call(n0=len(k0) - 1) == bad and call(n1=len(k1) - 1) == bad and call(k0p=None) == bad and call(k1p=None) == bad
    # nothing was written by a refused call, and the thread's source was not read
    assert n.value == 12345 and found.value == 55 and it.value == 99 and run.value == 77 and np.all(f == 7.0)
    assert not out.view(np.uint8).any()
    assert _color(amd) == fresh
    # accepted: max_trials at the limit is not refused as such (0 trials here), an epsilon the refit would refuse without a refit,
    # the four trailing pointers NULL
    assert call(opt=good.copy(max_trials=0, confidence=0.999999)) == 0 and run.value == 0
    assert call(opt=good.copy(epsilon_inliers=float("inf"))) == 0
    assert L.akz_remove_outliers_seeded(k0.ctypes.data, len(k0), k1.ctypes.data, len(k1), raw.ctypes.data, len(raw), C.byref(good), 0,
                                        out.ctypes.data, C.byref(n), None, None, None, None) == 0
    assert n.value <= len(raw)
