"""The seeded RANSAC on the GPU (akz_match_features_seeded_pairs): every pair's result equals the host statement
akz_remove_outliers_seeded on the pair's raw descriptor_match list with stream = stream_base + pair, bit for bit -- list, model
bits, found, accepted fits, trials run -- at the edges of K, of a wave, of the 256-lane tree, of a wave's 16 trials, of a round,
of the 8-round window and of two windows, with and without the stopping rule and the refit; the batch equals the loop of one-pair
calls; the guided stage gates with the model the call returns; refusals come before any GPU work; a second context runs it beside
an extraction.  Small planted-descriptor sets throughout: descriptor_match returns exactly the planted matches."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_fundamental_refit import SEEDS as SEEDS_F
from test_gpu_match_pairs import _color
from test_seeded_ransac_host import EARLY, EARLY_H, EPS, FULL, K, KIND, options, planted, same4

pytestmark = pytest.mark.gpu

RATIO = 0.86
SIZES = {"H": [3, 4, 5, 63, 64, 65, 255, 256, 257, 1000], "F": [7, 8, 9, 63, 64, 65, 255, 256, 257, 1000]}
# (max_trials, confidence, refine_iterations): every max_trials and every confidence the statement's edges ask for, the refit on
# and off at each kind of edge; the cross product is pruned to this list, which every size of both models runs
GRID = [(0, 0.99, 2), (1, 0.0, 2), (15, 0.5, 0), (16, 0.0, 0), (17, 0.99, 2), (127, 0.999999, 0), (128, 0.5, 2), (129, 0.0, 0),
        (1000, 0.0, 0), (1000, 0.99, 2), (1025, 0.999999, 0), (1025, 0.5, 2), (2177, 0.0, 2), (2177, 0.99, 0), (2177, 0.999999, 2)]


def seed_of(model, n):
    return SEEDS_F[n] if model == "F" else 500 + n


@pytest.fixture(scope="module")
def cases(amd):
    """one planted case per model and size, with its planted raw list (built once, left unchanged)"""
    return {(model, n): planted(amd, model, n, seed_of(model, n)) for model in SIZES for n in SIZES[model]}


def grid_epsilon(model, conf):
    """the fundamental matrix's winners keep ~8 matches at the refit tests' epsilon and never reach their count: with the rule on
    its cases run at epsilon 4, where they stop in different rounds (see test_seeded_ransac_host.py)"""
    return 4.0 if model == "F" and conf > 0 else EPS[model]


@pytest.mark.parametrize("model,n", [(m, n) for m in ("H", "F") for n in SIZES[m]])
def test_device_equals_host_statement(ctx, amd, cases, model, n):
    fa, fb, raw = cases[(model, n)]
    got_raw = ctx.descriptor_match(fa[1], fb[1], 10000, RATIO)
    assert np.array_equal(got_raw["index_0"], raw["index_0"]) and np.array_equal(got_raw["index_1"], raw["index_1"])
    stopped_early = ran_out = 0
    for max_trials, conf, its in GRID:
        opt = options(amd, model, max_trials=max_trials, confidence=conf, refine_iterations=its, stream_base=3,
                      epsilon_inliers=grid_epsilon(model, conf), lowes_ratio=RATIO)
        amd.random_seed(42, 69)
        fresh = _color(amd)
        amd.random_seed(42, 69)
        got = ctx.match_features_seeded_pairs([fa, fb], [(0, 1)], opt)[0]
        assert _color(amd) == fresh, (max_trials, conf, its)      # the thread's source: neither read nor advanced
        exp = amd.remove_outliers_seeded(fa[0], fb[0], got_raw, opt, stream=3)
        same4(got, exp, (model, n, max_trials, conf, its))
        run = got[3]
        if n < K[model]:
            assert run == 0 and got[1] is None and np.array_equal(got[0], got_raw)
        elif conf == 0.0:
            assert run == max_trials
        else:
            assert run <= max_trials and (run == max_trials or run % amd.RANSAC_ROUND == 0)
            stopped_early += run < max_trials
            ran_out += run == max_trials and max_trials > amd.RANSAC_ROUND
    if n >= 63:
        assert stopped_early > 0, (model, n)                      # (both branches of the rule were taken on this size)
    if model == "F" and n >= 257:
        assert ran_out > 0, (model, n)


def test_the_two_branches_chosen_on_the_host(ctx, amd):
    for (model, n, seed, kw, stream), want in ((EARLY, 3 * 128), (EARLY_H, 128), (FULL, FULL[3]["max_trials"])):
        fa, fb, raw = planted(amd, model, n, seed)
        for its in (0, 2):
            opt = options(amd, model, stream_base=stream, refine_iterations=its, lowes_ratio=RATIO, **kw)
            got = ctx.match_features_seeded_pairs([fa, fb], [(0, 1)], opt)[0]
            same4(got, amd.remove_outliers_seeded(fa[0], fb[0], ctx.descriptor_match(fa[1], fb[1], 10000, RATIO), opt, stream=stream),
                  (model, its))
            assert got[1] is not None and got[3] == want, (model, its, got[3])
            same4(amd.match_features_seeded(fa[0], fa[1], fb[0], fb[1], opt, ctx=ctx), got, "one pair")


def _pair_sets(amd, cases, model, nb=61):
    """sets 0 / 1, 2 / 3, 4 / 5: planted cases of 257, 65 and K - 1 matches; set 6: 300 rows unrelated to all; set 7: empty"""
    small = K[model] - 1
    if nb == 61:
        feats = [f for n in (257, 65, small) for f in cases[(model, n)][:2]]
    else:
        from test_gpu_fundamental_refit import planted_case as pf
        from test_gpu_homography_refit import planted_case as ph
        feats = [f for n in (257, 65, small) for f in (pf if model == "F" else ph)(amd, n, seed_of(model, n), nb=nb)[:2]]
    rng = np.random.default_rng(99)
    k = np.zeros(300, amd.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 1920, 300), rng.uniform(0, 1080, 300)
    feats.append((k, rng.integers(0, 256, (300, nb), dtype=np.uint8)))
    feats.append((np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, nb), np.uint8)))
    # a repeated pair, both orders, an (a, a) pair, unrelated sets, a pair below K, an empty set on either side, and the repeated
    # pair four more times: on the same raw list the streams stop in different rounds
    pairs = [(0, 1), (2, 3), (0, 1), (1, 0), (2, 2), (0, 6), (4, 5), (0, 7), (7, 2), (0, 1), (0, 1), (0, 1), (3, 2)]
    return feats, pairs


@pytest.mark.parametrize("model,nb,conf,its", [("H", 61, 0.999999, 2), ("F", 61, 0.99, 0), ("F", 64, 0.99, 2), ("H", 64, 0.0, 0)])
def test_batch_equals_the_loop_of_one_pair_calls(ctx, amd, cases, model, nb, conf, its):
    feats, pairs = _pair_sets(amd, cases, model, nb)
    opt = options(amd, model, max_trials=1025, confidence=conf, refine_iterations=its, stream_base=(1 << 64) - 3, lowes_ratio=RATIO,
                  epsilon_inliers=grid_epsilon(model, conf))
    amd.random_seed(42, 69)
    fresh = _color(amd)
    amd.random_seed(42, 69)
    got = ctx.match_features_seeded_pairs(feats, pairs, opt)
    assert len(got) == len(pairs)
    for p, (a, b) in enumerate(pairs):
        one = opt.copy(stream_base=(opt.stream_base + p) & ((1 << 64) - 1))     # (the stream wraps as u64)
        same4(got[p], ctx.match_features_seeded_pairs([feats[a], feats[b]], [(0, 1)], one)[0], ("loop", p))
        raw = ctx.descriptor_match(feats[a][1], feats[b][1], 10000, RATIO)
        same4(got[p], amd.remove_outliers_seeded(feats[a][0], feats[b][0], raw, opt, stream=one.stream_base), ("host", p))
    assert _color(amd) == fresh
    assert all(got[p][1] is not None for p in (0, 1, 2, 3, 9, 10, 11, 12))
    assert got[6][1] is None and got[6][3] == 0 and len(got[6][0]) == K[model] - 1        # below K: unchanged, nothing run
    assert got[7][3] == 0 and len(got[7][0]) == 0 and got[8][3] == 0 and len(got[8][0]) == 0
    if model == "F":   # (a, a): equal points give design rows of rank 6, no trial has a model; the zero model keeps every match
        assert got[4][1] is None and len(got[4][0]) == 65 and got[4][3] == 1025
    # the repeated pair: the same raw list, other streams -- other samples, so another winner or another number of trials
    if its == 0:       # (a refit may take different winners to one model)
        same = [p for p in (2, 9, 10, 11) if np.array_equal(got[p][1], got[0][1]) and got[p][3] == got[0][3]]
        assert not same, same
    if conf > 0 and model == "F":                                                         # (the homography's all stop after one round)
        assert len({got[p][3] for p in (0, 2, 9, 10, 11, 1, 12)}) >= 2                    # pairs that stop in different rounds
    elif conf == 0:
        assert all(got[p][3] == 1025 for p in (0, 1, 2, 3, 9, 10, 11, 12))
    twin = amd.match_features_seeded_pairs(feats, pairs[:3], opt, ctx=ctx)
    for g, e in zip(twin, got[:3]):
        same4(g, e, "twin")


@pytest.mark.parametrize("model,its", [("H", 0), ("H", 2), ("F", 0), ("F", 2)])
def test_guided_stage(ctx, amd, cases, model, its):
    feats, pairs = _pair_sets(amd, cases, model)
    n_guided = 0
    for radius, gratio in ((3.0, RATIO), (1.0, 0.95)):
        plain = options(amd, model, max_trials=300, refine_iterations=its, stream_base=11, lowes_ratio=RATIO,
                        epsilon_inliers=grid_epsilon(model, 0.99))
        ref = ctx.match_features_seeded_pairs(feats, pairs, plain)
        got = ctx.match_features_seeded_pairs(feats, pairs, plain.copy(guided=1, guided_radius=radius, guided_lowes_ratio=gratio))
        for p, ((a, b), g, r) in enumerate(zip(pairs, got, ref)):
            fa, fb = feats[a], feats[b]
            em = r[0] if r[1] is None else amd.descriptor_match_guided_host(fa[0], fa[1], fb[0], fb[1], r[1], KIND[model], radius, 10000,
                                                                           gratio)
            same4(g, (em, *r[1:]), (p, radius))     # found = 0: the unguided list; the model, the fits and the trials are the plain call's
            n_guided += r[1] is not None
    assert n_guided >= 12


def test_refusals_come_before_any_gpu_work(ctx, amd, cases):
    feats, pairs = _pair_sets(amd, cases, "F")
    good = options(amd, "F", max_trials=128)
    more = list(feats)
    more[3] = (feats[3][0][:10], feats[3][1])              # more descriptors than keypoints, in the second pair
    calls = [(feats, pairs, None), (feats, pairs, good.copy(struct_size=72)), (feats, pairs, good.copy(model_kind=7)),
             (feats, pairs, good.copy(max_trials=(1 << 24) + 1)), (feats, pairs, good.copy(confidence=1.0)),
             (feats, pairs, good.copy(confidence=-1e-9)), (feats, pairs, good.copy(confidence=float("nan"))),
             (feats, pairs, good.copy(guided=1, guided_radius=-1.0)), (feats, pairs, good.copy(guided=1, guided_radius=float("nan"))),
             (feats, pairs + [(0, 9)], good), (more, pairs, good)]
    amd.random_seed(42, 69)
    fresh = _color(amd)
    L = amd.lib()
    for k, (fs, pr, opt) in enumerate(calls):
        a = amd._PairsArgs(ctx, fs, pr)
        a.out["index_0"], a.n[:] = 77, 12345
        f = np.full((len(a.pr), 9), 7.0, np.float32)
        found, it, run = (np.full(len(a.pr), 55, t) for t in (np.int32, np.uint32, np.uint64))
        amd.random_seed(42, 69)
        status = L.akz_match_features_seeded_pairs(*a.head, C.byref(opt) if opt is not None else None, *a.tail,
                                                   f.ctypes.data_as(C.POINTER(C.c_float)), found.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   it.ctypes.data_as(C.POINTER(C.c_uint32)), run.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert status != 0, k
        assert np.all(a.out["index_0"] == 77) and np.all(a.n == 12345) and np.all(f == 7.0), k    # nothing was written
        assert np.all(found == 55) and np.all(it == 55) and np.all(run == 55), k
        assert _color(amd) == fresh, k
    with pytest.raises(amd.AkazeError):
        ctx.match_features_seeded_pairs(feats, pairs, good.copy(confidence=2.0))
    # an epsilon that the host statement's refit refuses is not refused here; NULL outputs are allowed
    ctx.match_features_seeded_pairs(feats, pairs[:2], good.copy(refine_iterations=2, epsilon_inliers=float("inf")))
    a = amd._PairsArgs(ctx, feats, pairs[:2])
    assert L.akz_match_features_seeded_pairs(*a.head, C.byref(good), *a.tail, None, None, None, None) == 0
    assert int(a.n[0]) <= 257


def test_second_context_beside_extraction(ctx, amd, cases):
    import torch
    other = amd.Context(0, torch.cuda.Stream().cuda_stream)
    try:
        runs = []
        for model in ("H", "F"):
            feats, pairs = _pair_sets(amd, cases, model)
            opt = options(amd, model, max_trials=1025, refine_iterations=2, lowes_ratio=RATIO, epsilon_inliers=grid_epsilon(model, 0.99))
            runs.append((feats, pairs, opt, ctx.match_features_seeded_pairs(feats, pairs, opt),
                         ctx.match_features_seeded_pairs(feats, pairs, opt.copy(guided=1))))
        frames = torch.from_numpy(np.stack([amd.synth_frame(1920, 1080, 40 + i) for i in range(4)])).cuda()
        job = ctx.extract_begin(frames, keep_all_planes=False)
        got = [(other.match_features_seeded_pairs(feats, pairs, opt), other.match_features_seeded_pairs(feats, pairs, opt.copy(guided=1)))
               for feats, pairs, opt, _, _ in runs]
        res = job.finish()
        assert res.counts(0)[1] > 0
        for (_, _, _, exp, exp_g), (g, gg) in zip(runs, got):
            for p, (x, e) in enumerate(zip(g, exp)):
                same4(x, e, p)
            for p, (x, e) in enumerate(zip(gg, exp_g)):
                same4(x, e, ("guided", p))
    finally:
        other.close()
