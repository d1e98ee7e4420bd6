"""The keypoint budget without a GPU: akz_keypoint_budget_host -- the statement of include/akaze_hip.h (AKZ_BUDGET_STRONGEST,
AKZ_BUDGET_SPREAD) -- against the same statement in numpy float32 (tests/budget_numpy.py), byte for byte: indices, n_out and
radius2.  Plus every refusal, each with its outputs untouched, and the declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from budget_numpy import F32, SPREAD, STRONGEST, budget_numpy, keypoints, lattice, random_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
AKZ_ERR_INVALID_ARG = -1
NEW_SYMBOLS = ("akz_keypoint_budget_host", "akz_keypoint_budget_sets")
DEBUG_SYMBOLS = ("akz_debug_keypoint_budget_split", "akz_debug_keypoint_budget_tiles")


def same(amd, kp, max_keypoints, mode, robust=0.9, what=None):
    """the library's statement and numpy's agree byte for byte; -> (indices, radius2)"""
    idx, rad = amd.keypoint_budget_host(kp, max_keypoints, mode, robust)
    eidx, erad = budget_numpy(kp, max_keypoints, mode, robust)
    assert idx.dtype == np.uint64 and len(idx) == min(int(max_keypoints), len(kp)), (what, len(idx))
    assert np.array_equal(idx, eidx), (what, max_keypoints, mode, idx[:8], eidx[:8])
    assert np.all(np.diff(idx.astype(np.int64)) > 0), what
    if mode == SPREAD:
        assert rad.dtype == F32 and rad.tobytes() == erad.tobytes(), (what, rad[:8], erad[:8])
    else:
        assert rad is None
    return idx, rad


def budgets(n):
    return sorted({0, 1, max(n - 1, 0), n, n + 5})


def test_symbols_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "akaze_hip_debug.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    for name in DEBUG_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", dbg) and name not in hdr, name
    assert re.search(r"#define\s+AKZ_BUDGET_STRONGEST\s+0\b", hdr) and re.search(r"#define\s+AKZ_BUDGET_SPREAD\s+1\b", hdr)
    assert "typedef struct akz_keypoint_budget" in hdr
    assert (amd.BUDGET_STRONGEST, amd.BUDGET_SPREAD) == (0, 1)
    assert C.sizeof(amd.KeypointBudget) == 16
    assert L.akz_abi_version() == 6
    for name in ("keypoint_budget_host", "limit_features"):
        assert callable(getattr(amd, name)), name
    assert callable(amd.Context.keypoint_budget_sets)
    q, t = amd.keypoint_budget_tiles()
    assert q >= 64 and t >= 64


@pytest.mark.parametrize("mode", [STRONGEST, SPREAD])
def test_tiny_sets(amd, mode):
    """n = 0, 1, 2 with max_keypoints = 0, 1, n - 1, n, n + 5"""
    for n in (0, 1, 2):
        kp = keypoints(amd, np.arange(n, dtype=F32) * 3, np.zeros(n, F32), np.asarray([0.5, 0.7][:n], F32))
        for m in budgets(n):
            idx, rad = same(amd, kp, m, mode, what=("tiny", n, m))
            if mode == SPREAD:
                assert len(rad) == n
    if mode == SPREAD:  # two keypoints: the weaker one (index 0) is suppressed at 3^2, the stronger one by nobody
        kp = keypoints(amd, [0, 3], [0, 0], [0.5, 0.7])
        idx, rad = same(amd, kp, 1, mode)
        assert list(idx) == [1] and list(rad) == [9.0, np.inf]


@pytest.mark.parametrize("mode", [STRONGEST, SPREAD])
@pytest.mark.parametrize("n", [37, 400])
def test_lattice_with_ties(amd, mode, n):
    kp = lattice(amd, n, seed=n + mode)
    for m in budgets(n) + [n // 2, n // 3]:
        same(amd, kp, m, mode, what=("lattice", n, m))
    if mode == SPREAD and n >= 400:  # the ties are there: few distinct radii, four responses
        _, rad = amd.keypoint_budget_host(kp, n, SPREAD, 0.9)
        assert len(np.unique(rad)) < n // 4 and len(np.unique(kp["response"])) == 4


@pytest.mark.parametrize("robust", [0.9, 1.0])
def test_equal_responses_dominate_nobody(amd, robust):
    """all responses equal: r < robust * r never holds for r > 0, every radius is +inf and the first N indices are kept"""
    kp = lattice(amd, 101, seed=3, values=(0.5, 0.5, 0.5, 0.5))
    for m in budgets(101) + [40]:
        idx, rad = same(amd, kp, m, SPREAD, robust, what=("equal", m))
        assert np.all(np.isinf(rad)) and list(idx) == list(range(min(m, 101)))
        idx, _ = same(amd, kp, m, STRONGEST, what=("equal", m))
        assert list(idx) == list(range(min(m, 101)))


def test_robust_exactly_one(amd):
    """robust = 1.0: j dominates i iff r_i < r_j, and equal responses do not suppress each other"""
    for n, seed in ((400, 5), (300, 6)):
        kp = lattice(amd, n, seed) if seed == 5 else random_set(amd, n, seed)
        for m in (1, n // 4, n - 1):
            same(amd, kp, m, SPREAD, 1.0, what=("robust 1", n, m))
    kp = keypoints(amd, [0, 1, 5], [0, 0, 0], [0.5, 0.5, 0.25])
    _, rad = same(amd, kp, 3, SPREAD, 1.0)
    assert list(rad) == [np.inf, np.inf, 16.0]


def test_duplicate_positions(amd):
    """coincident keypoints: d2 = 0, the weaker of a pair gets radius 0 and goes last"""
    rng = np.random.default_rng(8)
    base = random_set(amd, 120, 8)
    kp = np.concatenate([base, base[:60]])
    kp["response"][120:] = rng.permutation(kp["response"][:60])
    for m in budgets(180) + [60, 120]:
        same(amd, kp, m, SPREAD, what=("duplicates", m))
        same(amd, kp, m, STRONGEST, what=("duplicates", m))
    _, rad = amd.keypoint_budget_host(kp, 0, SPREAD, 0.9)
    assert np.count_nonzero(rad == 0) >= 30


def test_negative_and_signed_zero_responses(amd):
    """responses compare as values: -0 equals +0 (the index decides between them); a negative response dominates itself
    (r < robust * r), so its radius is 0"""
    r = np.asarray([0.0, -0.0, -0.5, 0.0, -0.0, 0.25, -0.25, -0.0, 0.0, -1.0], F32)
    rng = np.random.default_rng(9)
    kp = keypoints(amd, rng.integers(0, 6, len(r)).astype(F32), rng.integers(0, 6, len(r)).astype(F32), r)
    for m in range(len(r) + 2):
        same(amd, kp, m, STRONGEST, what=("signed", m))
        same(amd, kp, m, SPREAD, what=("signed", m))
    idx, _ = amd.keypoint_budget_host(kp, 5, STRONGEST)
    assert list(idx) == [0, 1, 3, 4, 5]  # 0.25, then the zeros of either sign in index order
    _, rad = amd.keypoint_budget_host(kp, 0, SPREAD, 0.9)
    assert all(rad[i] == 0 for i in (2, 6, 9))
    big = random_set(amd, 300, 10)
    big["response"] -= np.float32(np.median(big["response"]))
    for m in (1, 100, 299):
        same(amd, big, m, SPREAD, what=("negative", m))
        same(amd, big, m, STRONGEST, what=("negative", m))


@pytest.mark.parametrize("n", [300, 1500])
def test_random_sets(amd, n):
    kp = random_set(amd, n, seed=n)
    for m in (1, n // 10, n // 2, n - 1, n, n + 5):
        same(amd, kp, m, SPREAD, what=("random", n, m))
        same(amd, kp, m, STRONGEST, what=("random", n, m))
    same(amd, kp, n // 3, SPREAD, 0.5, what=("random robust 0.5", n))
    # subnormal distances and responses stay what they are
    tiny = random_set(amd, 64, seed=n + 1, w=1e-20, h=1e-20)
    tiny["response"] *= np.float32(1e-37)
    idx, rad = same(amd, tiny, 20, SPREAD, what="subnormal")
    assert np.any((rad > 0) & (rad < np.finfo(F32).tiny))


def test_oracle_keypoints_of_the_reference_image(amd, ref):
    """the keypoints the CPU oracle finds in tests/golden/1.jpg: a real distribution -- clustered, thousands, responses over decades"""
    luma = amd.load_image_luma(os.path.join(GOLDEN, "1.jpg"))
    kp = ref.extract(luma, threads=8).keypoints()
    assert len(kp) > 1000
    for m in (500, 1000):
        idx, _ = same(amd, kp, m, SPREAD, what=("1.jpg", m))
        sidx, _ = same(amd, kp, m, STRONGEST, what=("1.jpg", m))
        assert not np.array_equal(idx, sidx)


def test_refusals_write_nothing(amd):
    L = amd.lib()
    kp = random_set(amd, 16, 1)
    kpp = kp.ctypes.data_as(C.c_void_p)

    def call(k=kpp, n=16, opt=amd.KeypointBudget(8, SPREAD, 0.9), with_idx=True, with_n=True, with_rad=True, word=None):
        idx = np.full(16, 0x5a5a5a5a5a5a5a5a, np.uint64)
        rad = np.full(16, -7.0, F32)
        cnt = C.c_uint64(77)
        st = L.akz_keypoint_budget_host(k, n, C.byref(opt) if opt is not None else None, idx.ctypes.data_as(C.c_void_p) if with_idx else None,
                                        C.byref(cnt) if with_n else None, rad.ctypes.data_as(C.c_void_p) if with_rad else None)
        msg = L.akz_last_error().decode()
        assert st == AKZ_ERR_INVALID_ARG, (st, msg)
        assert msg.startswith("keypoint_budget_host: ") and (word is None or word in msg), msg
        assert np.all(idx == 0x5a5a5a5a5a5a5a5a) and np.all(rad == -7.0) and cnt.value == 77, msg
        return msg

    call(opt=None, word="null")
    call(opt=amd.KeypointBudget(8, 2, 0.9), word="mode")
    call(opt=amd.KeypointBudget(8, 0xffffffff, 0.9), word="mode")
    for robust in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        call(opt=amd.KeypointBudget(8, SPREAD, robust), word="robust")
    for field in ("x", "y", "response"):
        for bad in (np.nan, np.inf, -np.inf):
            k = kp.copy()
            k[field][11] = bad
            call(k=k.ctypes.data_as(C.c_void_p), word="keypoint 11")
    call(k=None, word="null keypoints")
    call(with_idx=False, word="null")
    call(with_n=False, word="null")
    call(opt=amd.KeypointBudget(8, STRONGEST, 0.9), word="radius2")
    call(n=1 << 31, word="2^31 - 1")  # (refused before a keypoint is read)
    # ... and what is not refused: robust is not read in STRONGEST mode, n = 0 needs no keypoints, max_keypoints = 0 is fine
    idx = np.zeros(16, np.uint64)
    cnt = C.c_uint64(77)
    opt = amd.KeypointBudget(8, STRONGEST, float("nan"))
    assert L.akz_keypoint_budget_host(kpp, 16, C.byref(opt), idx.ctypes.data_as(C.c_void_p), C.byref(cnt), None) == 0 and cnt.value == 8
    opt = amd.KeypointBudget(8, SPREAD, 1.0)
    assert L.akz_keypoint_budget_host(None, 0, C.byref(opt), idx.ctypes.data_as(C.c_void_p), C.byref(cnt), None) == 0 and cnt.value == 0
    opt = amd.KeypointBudget(0, SPREAD, 0.9)
    rad = np.full(16, -7.0, F32)
    assert L.akz_keypoint_budget_host(kpp, 16, C.byref(opt), idx.ctypes.data_as(C.c_void_p), C.byref(cnt), rad.ctypes.data_as(C.c_void_p)) == 0
    assert cnt.value == 0 and np.all(rad >= 0)


def test_sets_call_refusals_reach_no_gpu(amd):
    """akz_keypoint_budget_sets: every refusal comes before any GPU work -- a NULL context is refused first, so none of these
    calls can have touched a device -- and n_sets = 0 is AKZ_OK without one"""
    L = amd.lib()
    kp = random_set(amd, 16, 2)
    sets = (amd.FeatureSet * 2)(amd.FeatureSet(kp.ctypes.data_as(C.c_void_p), 16, None, 0), amd.FeatureSet(None, 0, None, 0))
    idx = np.full(16, 7, np.uint64)
    cnt = np.full(2, 77, np.uint64)
    opt = amd.KeypointBudget(8, SPREAD, 0.9)
    args = (C.byref(opt), idx.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), None)
    assert L.akz_keypoint_budget_sets(None, C.cast(sets, C.c_void_p), 2, *args) == AKZ_ERR_INVALID_ARG
    assert "null context" in L.akz_last_error().decode()
    assert L.akz_keypoint_budget_sets(None, C.cast(sets, C.c_void_p), 0, *args) == 0
    assert L.akz_keypoint_budget_sets(None, None, 0, None, None, None, None) == 0
    assert np.all(idx == 7) and np.all(cnt == 77)
