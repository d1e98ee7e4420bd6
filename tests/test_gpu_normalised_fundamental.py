"""The third model kind of the seeded RANSAC on the GPU (AKZ_RANSAC_FUNDAMENTAL_NORMALISED through
akz_match_features_seeded_pairs): every pair's result equals the host statement akz_remove_outliers_seeded on the pair's raw
descriptor_match list with stream = stream_base + pair, bit for bit -- list, model bits, found, accepted fits, trials run -- at
the edges of K, of a wave and of the 256-lane tree, over the (max_trials, confidence, refit) grid of test_gpu_seeded_ransac.py at
2 px; the batch equals the loop; the one-wave kernels of 64 pairs and more; the guided stage gates with the returned F as an
epipolar band; refusals come before any GPU work; kinds 0 and 1 beside it in the same process.  Small planted-descriptor sets
throughout: descriptor_match returns exactly the planted matches."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_fundamental_refit import SEEDS
from test_gpu_match_pairs import _color
from test_gpu_seeded_ransac import GRID, RATIO, _pair_sets
from test_normalised_fundamental_host import BRANCH_SCENE, EPS, FIRST, LATER, OUT, nopt, sampson_rule
from test_seeded_ransac_host import options, planted, same4

pytestmark = pytest.mark.gpu

SIZES = [7, 8, 9, 63, 64, 65, 255, 256, 257, 1000]   # the edges of K = 8, of a wave and of the 256-lane tree
# Beside the grid at 2 px, where every size from 63 up stops after its first or second round: one entry at a quarter of a pixel
# (a third of the noise), where the best of 1 000 trials stays below its count on each of those sizes (found on the host, see
# test_normalised_fundamental_host.py) -- so both branches of the rule are taken on every size
SUB_PIXEL = (1000, 0.99, 2, 0.25)


@pytest.fixture(scope="module")
def cases(amd):
    """one planted case per size with its planted raw list, under the key _pair_sets wants (built once, left unchanged)"""
    return {("F", n): planted(amd, "F", n, SEEDS[n]) for n in SIZES}


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host_statement(ctx, amd, cases, n):
    fa, fb, raw = cases[("F", n)]
    got_raw = ctx.descriptor_match(fa[1], fb[1], 10000, RATIO)
    assert np.array_equal(got_raw["index_0"], raw["index_0"]) and np.array_equal(got_raw["index_1"], raw["index_1"])
    stopped_early = ran_out = 0
    for max_trials, conf, its, eps in [(*g, EPS) for g in GRID] + [SUB_PIXEL]:
        opt = nopt(amd, max_trials=max_trials, confidence=conf, refine_iterations=its, stream_base=3, epsilon_inliers=eps, lowes_ratio=RATIO)
        amd.random_seed(42, 69)
        fresh = _color(amd)
        amd.random_seed(42, 69)
        got = ctx.match_features_seeded_pairs([fa, fb], [(0, 1)], opt)[0]
        assert _color(amd) == fresh, (max_trials, conf, its)      # the thread's source: neither read nor advanced
        exp = amd.remove_outliers_seeded(fa[0], fb[0], got_raw, opt, stream=3)
        same4(got, exp, (n, max_trials, conf, its, eps))
        kept, f, done, run = got
        if n < 8:
            assert run == 0 and f is None and np.array_equal(kept, got_raw)
            continue
        assert np.array_equal(kept, got_raw[sampson_rule(f, fa[0], fb[0], got_raw, eps)])    # (no winner: the zero model, nothing)
        assert done <= its
        if n >= 63:
            assert (f is None) == (max_trials == 0)
        if conf == 0.0:
            assert run == max_trials
        else:
            assert run <= max_trials and (run == max_trials or run % amd.RANSAC_ROUND == 0)
            stopped_early += run < max_trials
            ran_out += run == max_trials and max_trials > amd.RANSAC_ROUND
    if n >= 63:
        assert stopped_early > 0 and ran_out > 0, (n, stopped_early, ran_out)


def test_the_three_branches_chosen_on_the_host(ctx, amd):
    fa, fb, raw = planted(amd, "F", *BRANCH_SCENE)
    got_raw = ctx.descriptor_match(fa[1], fb[1], 10000, RATIO)
    for kw, stream, want in (FIRST, LATER, OUT):
        for its in (0, 2):
            opt = nopt(amd, stream_base=stream, refine_iterations=its, lowes_ratio=RATIO, **kw)
            got = ctx.match_features_seeded_pairs([fa, fb], [(0, 1)], opt)[0]
            same4(got, amd.remove_outliers_seeded(fa[0], fb[0], got_raw, opt, stream=stream), (want, its))
            assert got[1] is not None and got[3] == want, (want, its, got[3])
            same4(amd.match_features_seeded(fa[0], fa[1], fb[0], fb[1], opt, ctx=ctx), got, "one pair")


@pytest.mark.parametrize("nb,conf,its", [(61, 0.99, 0), (64, 0.999999, 2), (61, 0.0, 2)])
def test_batch_equals_the_loop_of_one_pair_calls(ctx, amd, cases, nb, conf, its):
    feats, pairs = _pair_sets(amd, cases, "F", nb)
    opt = nopt(amd, max_trials=1025, confidence=conf, refine_iterations=its, stream_base=(1 << 64) - 3, lowes_ratio=RATIO)
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
    assert got[6][1] is None and got[6][3] == 0 and len(got[6][0]) == 7                    # below K: unchanged, nothing run
    assert got[7][3] == 0 and len(got[7][0]) == 0 and got[8][3] == 0 and len(got[8][0]) == 0
    # (a, a): equal points in both images leave a null space of three dimensions, the rank rule refuses every sample; the zero
    # model keeps nothing under the Sampson rule
    assert got[4][1] is None and len(got[4][0]) == 0 and got[4][3] == 1025
    if its == 0:       # the repeated pair: the same raw list, other streams -- other samples, so another winner
        same = [p for p in (2, 9, 10, 11) if np.array_equal(got[p][1], got[0][1])]
        assert not same, same
    if conf == 0:
        assert all(got[p][3] == 1025 for p in (0, 1, 2, 3, 9, 10, 11, 12))
    else:
        assert all(got[p][3] < 1025 for p in (0, 1, 2, 3, 9, 10, 11, 12))    # at 2 px every pair reaches its count
    twin = amd.match_features_seeded_pairs(feats, pairs[:3], opt, ctx=ctx)
    for g, e in zip(twin, got[:3]):
        same4(g, e, "twin")


@pytest.mark.parametrize("max_trials,conf,its", [(129, 0.0, 2), (300, 0.99, 0)])
def test_the_one_wave_kernels(ctx, amd, cases, max_trials, conf, its):
    """64 pairs are 512 workgroups a round: the kernels without helper waves.  64 copies of the 65-match pair and two more."""
    fa, fb, _ = cases[("F", 65)]
    fc, fd, _ = cases[("F", 257)]
    feats = [fa, fb, fc, fd]
    pairs = [(0, 1)] * 64 + [(2, 3), (1, 0)]
    opt = nopt(amd, max_trials=max_trials, confidence=conf, refine_iterations=its, stream_base=21, lowes_ratio=RATIO)
    got = ctx.match_features_seeded_pairs(feats, pairs, opt)
    raws = {pr: ctx.descriptor_match(feats[pr[0]][1], feats[pr[1]][1], 10000, RATIO) for pr in set(pairs)}
    for p, (a, b) in enumerate(pairs):
        same4(got[p], amd.remove_outliers_seeded(feats[a][0], feats[b][0], raws[(a, b)], opt, stream=21 + p), p)
        assert got[p][1] is not None
    few = ctx.match_features_seeded_pairs(feats, pairs[:3] + pairs[-2:], opt.copy(stream_base=21))   # the helper-wave kernels
    for g, e in zip(few[:3], got[:3]):
        same4(g, e, "helper waves")


@pytest.mark.parametrize("its", [0, 2])
def test_guided_stage(ctx, amd, cases, its):
    feats, pairs = _pair_sets(amd, cases, "F")
    n_guided = 0
    for radius, gratio in ((3.0, RATIO), (1.0, 0.95)):
        plain = nopt(amd, max_trials=300, refine_iterations=its, stream_base=11, lowes_ratio=RATIO)
        ref = ctx.match_features_seeded_pairs(feats, pairs, plain)
        got = ctx.match_features_seeded_pairs(feats, pairs, plain.copy(guided=1, guided_radius=radius, guided_lowes_ratio=gratio))
        for p, ((a, b), g, r) in enumerate(zip(pairs, got, ref)):
            fa, fb = feats[a], feats[b]
            em = r[0] if r[1] is None else amd.descriptor_match_guided(fa[0], fa[1], fb[0], fb[1], r[1], amd.GUIDED_FUNDAMENTAL, radius,
                                                                       10000, gratio, ctx=ctx)
            same4(g, (em, *r[1:]), (p, radius))     # found = 0: the unguided list; the model, the fits and the trials are the plain call's
            if r[1] is not None:
                host = amd.descriptor_match_guided_host(fa[0], fa[1], fb[0], fb[1], r[1], amd.GUIDED_FUNDAMENTAL, radius, 10000, gratio)
                assert np.array_equal(em, host), p
            n_guided += r[1] is not None
    assert n_guided >= 16


def test_refusals_come_before_any_gpu_work(ctx, amd, cases):
    feats, pairs = _pair_sets(amd, cases, "F")
    good = nopt(amd, max_trials=128)
    calls = [good.copy(model_kind=2), good.copy(model_kind=7), good.copy(model_kind=-1), good.copy(model_kind=4),
             good.copy(struct_size=72), good.copy(confidence=1.0), good.copy(max_trials=(1 << 24) + 1),
             good.copy(guided=1, guided_radius=-1.0)]
    amd.random_seed(42, 69)
    fresh = _color(amd)
    L = amd.lib()
    for k, opt in enumerate(calls):
        a = amd._PairsArgs(ctx, feats, pairs)
        a.out["index_0"], a.n[:] = 77, 12345
        f = np.full((len(a.pr), 9), 7.0, np.float32)
        found, it, run = (np.full(len(a.pr), 55, t) for t in (np.int32, np.uint32, np.uint64))
        amd.random_seed(42, 69)
        status = L.akz_match_features_seeded_pairs(*a.head, C.byref(opt), *a.tail, f.ctypes.data_as(C.POINTER(C.c_float)),
                                                   found.ctypes.data_as(C.POINTER(C.c_int32)), it.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                   run.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert status != 0, k
        assert np.all(a.out["index_0"] == 77) and np.all(a.n == 12345) and np.all(f == 7.0), k    # nothing was written
        assert np.all(found == 55) and np.all(it == 55) and np.all(run == 55), k
        assert _color(amd) == fresh, k
    # the guided calls know two kinds, as before
    fa, fb = feats[0], feats[1]
    model = ctx.match_features_seeded_pairs(feats, pairs[:1], good)[0][1]
    assert model is not None
    amd.random_seed(42, 69)                                    # (_color draws from the source: reseed before it is read again)
    for kind in (amd.RANSAC_FUNDAMENTAL_NORMALISED, 2):
        with pytest.raises(amd.AkazeError):
            amd.descriptor_match_guided(fa[0], fa[1], fb[0], fb[1], model, kind, 3.0, 10000, RATIO, ctx=ctx)
        with pytest.raises(amd.AkazeError):
            ctx.descriptor_match_guided_pairs(feats, pairs[:1], [model], kind, 3.0, 10000, RATIO)
    assert _color(amd) == fresh
    # an epsilon that the host statement's refit refuses is not refused here; NULL outputs are allowed
    ctx.match_features_seeded_pairs(feats, pairs[:2], good.copy(refine_iterations=2, epsilon_inliers=float("inf")))
    a = amd._PairsArgs(ctx, feats, pairs[:2])
    assert L.akz_match_features_seeded_pairs(*a.head, C.byref(good), *a.tail, None, None, None, None) == 0
    assert int(a.n[0]) <= 257


@pytest.mark.parametrize("model", ["H", "F"])
def test_kinds_0_and_1_beside_it(ctx, amd, cases, model):
    """the other two kinds in the same process, between two calls of the new one: still what the host statement gives"""
    from test_gpu_seeded_ransac import grid_epsilon, seed_of
    fa, fb, raw = planted(amd, model, 257, seed_of(model, 257))
    na, nb, _ = cases[("F", 257)]
    new = nopt(amd, max_trials=1000, confidence=0.99, refine_iterations=2, stream_base=3, lowes_ratio=RATIO)
    before = ctx.match_features_seeded_pairs([na, nb], [(0, 1)], new)[0]
    got_raw = ctx.descriptor_match(fa[1], fb[1], 10000, RATIO)
    for max_trials, conf, its in ((1000, 0.99, 2), (129, 0.0, 0)):
        opt = options(amd, model, max_trials=max_trials, confidence=conf, refine_iterations=its, stream_base=3,
                      epsilon_inliers=grid_epsilon(model, conf), lowes_ratio=RATIO)
        got = ctx.match_features_seeded_pairs([fa, fb], [(0, 1)], opt)[0]
        same4(got, amd.remove_outliers_seeded(fa[0], fb[0], got_raw, opt, stream=3), (model, max_trials))
        assert got[1] is not None
    same4(ctx.match_features_seeded_pairs([na, nb], [(0, 1)], new)[0], before, "again")
