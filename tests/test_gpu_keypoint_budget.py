"""The keypoint budget on the GPU: Context.keypoint_budget_sets (akz_keypoint_budget_sets: k_budget_walk's radius and rank passes,
k_budget_compact) against the host statement akz_keypoint_budget_host, byte for byte -- indices, counts and radius2 -- in both modes;
the large sets against the numpy statement of tests/budget_numpy.py as well.  Set sizes sit one below, at and one above the walk's
LDS stage (256 keypoints) and its query tile (1 024), with empty sets first and in the middle."""
import ctypes as C
import os

import numpy as np
import pytest

from budget_numpy import F32, SPREAD, STRONGEST, budget_numpy, lattice, random_set

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SIZES = [0, 1, 2, 63, 64, 65, 0, 255, 256, 257, 1000, 2049]
MODES = [STRONGEST, SPREAD]


def host_sets(amd, sets, max_keypoints, mode, robust=0.9):
    return [amd.keypoint_budget_host(k, max_keypoints, mode, robust) for k in sets]


def same_sets(got, exp, what=None):
    assert len(got) == len(exp), what
    for s, ((gi, gr), (ei, er)) in enumerate(zip(got, exp)):
        assert gi.dtype == ei.dtype == np.uint64 and gi.tobytes() == ei.tobytes(), (what, s, len(gi), len(ei), gi[:8], ei[:8])
        assert (gr is None) == (er is None), (what, s)
        if gr is not None:
            assert gr.dtype == F32 and gr.tobytes() == er.tobytes(), (what, s, gr[:8], er[:8])


@pytest.fixture(scope="module")
def mixed(amd):
    """the sets of the one sets call: SIZES plus the sizes around the built kernel's query tile and LDS stage; alternately random
    floats and lattice-with-ties"""
    q, t = amd.keypoint_budget_tiles()
    sizes = list(SIZES)
    for edge in (t, q):
        sizes += [v for v in (edge - 1, edge, edge + 1) if v not in sizes]
    return [random_set(amd, n, 40 + i) if i % 2 else lattice(amd, n, 40 + i) for i, n in enumerate(sizes)]


@pytest.fixture(scope="module")
def big(amd):
    """one set of 4 097 on the lattice with ties, one of random floats; the host statement of both, computed once"""
    sets = {"lattice": lattice(amd, 4097, 7), "random": random_set(amd, 4097, 8)}
    exp = {(name, mode, m): amd.keypoint_budget_host(k, m, mode, 0.9)
           for name, k in sets.items() for mode in MODES for m in (1, 500, 4096)}
    return sets, exp


@pytest.mark.parametrize("mode", MODES)
def test_one_call_over_mixed_sets(amd, ctx, mixed, mode):
    for m in (0, 1, 100, 5000):
        same_sets(ctx.keypoint_budget_sets(mixed, m, mode, 0.9), host_sets(amd, mixed, m, mode), what=("mixed", mode, m))
    same_sets(ctx.keypoint_budget_sets([(k, None) for k in mixed], 300, mode, 1.0), host_sets(amd, mixed, 300, mode, 1.0), what="robust 1")
    assert ctx.keypoint_budget_sets([], 10, mode) == []
    (idx, rad), = ctx.keypoint_budget_sets([mixed[0]], 10, mode)
    assert len(idx) == 0 and (rad is None or len(rad) == 0)


@pytest.mark.parametrize("mode", MODES)
def test_lattice_with_ties_4097(amd, ctx, big, mode):
    sets, exp = big
    for m in (1, 500, 4096):
        same_sets(ctx.keypoint_budget_sets([sets["lattice"]], m, mode), [exp["lattice", mode, m]], what=("lattice", mode, m))


@pytest.mark.parametrize("mode", MODES)
def test_random_4097_against_host_and_numpy(amd, ctx, big, mode):
    sets, exp = big
    for m in (1, 500, 4096):
        got = ctx.keypoint_budget_sets([sets["random"]], m, mode)
        same_sets(got, [exp["random", mode, m]], what=("random", mode, m))
    same_sets(got, [budget_numpy(sets["random"], 4096, mode, 0.9)], what=("random against numpy", mode))


def calls_in_order(amd, c, mixed, big_sets):
    """a large job, then smaller ones, then the large one again -- each twice in a row; -> every result"""
    jobs = [([big_sets["random"], big_sets["lattice"]] + mixed, 700, SPREAD), (mixed[:6], 40, SPREAD), ([mixed[3]], 5, STRONGEST),
            (mixed, 200, STRONGEST), ([big_sets["random"], big_sets["lattice"]] + mixed, 700, SPREAD), ([mixed[-1]], 900, SPREAD)]
    out = []
    for sets, m, mode in jobs:
        first = c.keypoint_budget_sets(sets, m, mode)
        same_sets(c.keypoint_budget_sets(sets, m, mode), first, what=("twice in a row", len(sets), m, mode))
        out.append(first)
    return jobs, out


def test_smaller_job_after_larger(amd, ctx, mixed, big):
    """stale scratch does not leak: a smaller job after a larger one equals the host statement, and a repeated call itself"""
    jobs, out = calls_in_order(amd, ctx, mixed, big[0])
    for (sets, m, mode), got in zip(jobs[1:4], out[1:4]):
        same_sets(got, host_sets(amd, sets, m, mode), what=("after a larger job", len(sets), m, mode))
    same_sets(out[4], out[0], what="the large job again")


def test_filled_allocations(amd, ctx, mixed, big):
    """the same calls on a context whose fresh device memory holds 0xA5 bytes give the same bytes, and the scratch audit is clean"""
    import torch
    _, exp = calls_in_order(amd, ctx, mixed, big[0])
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        c.debug_set_alloc_fill(True)
        _, got = calls_in_order(amd, c, mixed, big[0])
        for g, e in zip(got, exp):
            same_sets(g, e, what="filled")
        rows = c.debug_audit_scratch()
        assert rows and all(r["first_bad"] is None for r in rows), rows
    finally:
        c.close()


def test_limit_features_feeds_the_pairs_calls(amd, ctx):
    """limit_features' output goes straight into match_features_seeded_pairs and gives what the numpy-gathered subsets give"""
    res = ctx.extract_features_files([os.path.join(GOLDEN, n) for n in ("1.jpg", "2.jpg")])
    feats = [(res.keypoints(i), res.descriptors(i)) for i in (0, 1)]
    assert min(len(k) for k, _ in feats) > 2000
    opt = amd.RansacOptions()
    for mode in MODES:
        cut, gathered = [], []
        for k, d in feats:
            kk, dd, idx = amd.limit_features(k, d, 1000, mode, 0.9, ctx=ctx)
            eidx, _ = budget_numpy(k, 1000, mode, 0.9)
            assert len(idx) == 1000 and np.array_equal(idx, eidx)
            assert kk.dtype == amd.KEYPOINT_DTYPE and dd.dtype == np.uint8 and dd.shape == (1000, d.shape[1])
            cut.append((kk, dd))
            gathered.append((k[eidx.astype(np.int64)], d[eidx.astype(np.int64)]))
        (gm, gf, gi, gt), = ctx.match_features_seeded_pairs(cut, [(0, 1)], opt)
        (em, ef, ei, et), = ctx.match_features_seeded_pairs(gathered, [(0, 1)], opt)
        # (the golden pair keeps raw matches at this budget in both modes, so equal lists are not two empty ones)
        assert len(em) > 0 and gm.tobytes() == em.tobytes() and (gi, gt) == (ei, et)
        assert (gf is None) == (ef is None) and (gf is None or np.asarray(gf).tobytes() == np.asarray(ef).tobytes())


def test_refusals_reach_no_gpu_work(amd, ctx):
    """every refusal of the statement through the sets call: AKZ_ERR_INVALID_ARG naming the set, nothing written -- also with a
    NULL context (refused itself while n_sets > 0), which no GPU work could have run on"""
    L = amd.lib()
    good = random_set(amd, 16, 1)
    bad = good.copy()
    bad["y"][5] = np.inf

    def refused(sets, opt, word, with_rad=False, h=ctx._h, with_idx=True):
        arr = (amd.FeatureSet * len(sets))(*[amd.FeatureSet(k.ctypes.data_as(C.c_void_p) if k is not None else None, n, None, 0)
                                             for k, n in sets])
        idx = np.full(64, 7, np.uint64)
        cnt = np.full(8, 77, np.uint64)
        rad = np.full(64, -7.0, F32)
        st = L.akz_keypoint_budget_sets(h, C.cast(arr, C.c_void_p), len(sets), C.byref(opt) if opt is not None else None,
                                        idx.ctypes.data_as(C.c_void_p) if with_idx else None, cnt.ctypes.data_as(C.c_void_p),
                                        rad.ctypes.data_as(C.c_void_p) if with_rad else None)
        msg = L.akz_last_error().decode()
        assert st == -1 and word in msg, (st, msg)
        assert np.all(idx == 7) and np.all(cnt == 77) and np.all(rad == -7.0), msg

    ok = amd.KeypointBudget(8, SPREAD, 0.9)
    two = [(good, 16), (good, 16)]
    refused(two, None, "null")
    refused(two, amd.KeypointBudget(8, 5, 0.9), "mode")
    refused(two, amd.KeypointBudget(8, SPREAD, 0.0), "robust")
    refused(two, amd.KeypointBudget(8, SPREAD, float("nan")), "robust")
    refused([(good, 16), (bad, 16)], ok, "set 1: keypoint 5")
    refused([(good, 16), (None, 3)], ok, "set 1: null keypoints")
    refused(two, ok, "null", with_idx=False)
    refused(two, amd.KeypointBudget(8, STRONGEST, 0.9), "radius2", with_rad=True)
    refused([(good, 16), (good, 1 << 31)], ok, "set 1: more than 2^31 - 1")
    refused([(good, (1 << 31) - 1), (good, 16)], amd.KeypointBudget(8, SPREAD, 2.0), "robust")
    refused(two, ok, "null context", h=None)
    # the context is as good as before
    same_sets(ctx.keypoint_budget_sets([good], 8, SPREAD), [amd.keypoint_budget_host(good, 8, SPREAD)])
