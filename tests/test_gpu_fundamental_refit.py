"""The fundamental matrix of match_features handed back, refitted and guiding, on the GPU (akz_match_features_fundamental and
its _refined / _guided / _pairs forms): the device result equals the host composite descriptor_match ->
remove_outliers_fundamental -> refine_fundamental_matrix on the raw list bit for bit (list, F, found, accepted fits, the random
source's state), the unrefined forms are match_features(_pairs) with the model, refine_iterations = 0 is the unrefined call, the
pairs call is the loop of the single call, the guided forms gate with the F they return, and a second context runs it beside
an extraction.  Small planted-descriptor sets of a two-view scene throughout: descriptor_match returns exactly the planted
matches."""
import numpy as np
import pytest

from test_fundamental_refit_host import EPS_MODEL, error_rule, two_view_scene
from test_gpu_homography import _hbits
from test_gpu_match_pairs import _color

pytestmark = pytest.mark.gpu

SIZES = [7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 3001]   # the edges of K = 8, of a wave, of the 256 lanes, of the tree
# scene seed per size.  From 63 up: the first seed from 500 + n on at which the host statement accepts two fits or more from
# the winner of 1 000 trials at EPS (found on the host with remove_outliers_fundamental and refine_fundamental_matrix on the
# planted list: the trial model often gives a winner that no refit improves, see test_fundamental_refit_host.py).
SEEDS = {7: 507, 8: 508, 9: 509, 63: 595, 64: 640, 65: 575, 255: 765, 256: 761, 257: 757, 511: 1014, 513: 1018, 1000: 1502,
         3001: 3502}
EPS = 0.02    # |p1^T F p0| at unit norm: 1 .. 5 px on these scenes
RATIO = 0.86


def planted_case(amd, n, seed, nb=61):
    """n keypoints per image of two_view_scene(seed, n) (0.7 px noise, 20 % outliers), keypoint i of image 0 matching keypoint
    perm[i] of image 1 through equal random descriptors.  Returns ((k0, d0), (k1, d1))."""
    sc = two_view_scene(seed, n)
    rng = np.random.default_rng(seed + 7)
    perm = rng.permutation(n)
    k0 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k1 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k0["x"], k0["y"] = sc[0][:, 0], sc[0][:, 1]
    k1["x"][perm], k1["y"][perm] = sc[2][:, 0], sc[2][:, 1]
    d0 = rng.integers(0, 256, (n, nb), dtype=np.uint8)
    d1 = np.zeros_like(d0)
    d1[perm] = d0
    return (k0, d0), (k1, d1)


@pytest.fixture(scope="module")
def cases(amd):
    """one planted case per size (built once, left unchanged)"""
    return {n: planted_case(amd, n, SEEDS[n]) for n in SIZES}


def _host(ctx, amd, fa, fb, ratio, trials, eps, its):
    """the host composite -> (list, F or None, accepted fits)"""
    raw = ctx.descriptor_match(fa[1], fb[1], 10000, ratio)
    kept, f = amd.remove_outliers_fundamental(fa[0], fb[0], raw, trials, EPS_MODEL, eps)
    if f is None or its == 0:
        return kept, f, 0
    return amd.refine_fundamental_matrix(fa[0], fb[0], raw, f, eps, its)


def _same3(got, exp, what):
    (gm, gf, gi), (em, ef, ei) = got, exp
    assert gm.dtype == em.dtype and np.array_equal(gm, em), (what, len(gm), len(em))
    assert (gf is None) == (ef is None), what
    if gf is not None:
        assert np.array_equal(_hbits(gf), _hbits(ef)), (what, gf, ef)
    assert gi == ei, (what, gi, ei)


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host_composite(ctx, amd, cases, n):
    fa, fb = cases[n]
    raw = ctx.descriptor_match(fa[1], fb[1], 10000, RATIO)
    assert len(raw) == n                                   # the planted matches, all of them
    fitted = False
    for trials in (0, 1, 1000):
        for its in (1, 2, 8):
            amd.random_seed(42, 69)
            got = amd.match_features_fundamental_refined(fa[0], fa[1], fb[0], fb[1], RATIO, trials, EPS, its, ctx=ctx)
            after_dev = _color(amd)
            amd.random_seed(42, 69)
            exp = _host(ctx, amd, fa, fb, RATIO, trials, EPS, its)
            after_host = _color(amd)
            _same3(got, exp, (n, trials, its))
            assert after_dev == after_host, (n, trials, its)
            assert got[2] <= its
            if trials == 0 or n < 8:
                assert got[1] is None and got[2] == 0 and np.array_equal(got[0], raw)
            if got[1] is not None:
                assert np.array_equal(got[0], raw[error_rule(got[1], fa[0], fb[0], raw, EPS)])
            fitted |= got[2] > 0
    if n >= 63:
        assert fitted, n                                   # (the stage did run a fit that was accepted)


@pytest.mark.parametrize("n", [7, 9, 257, 1000])
def test_unrefined_forms(ctx, amd, cases, n):
    """match_features_fundamental is match_features with the model; refine_iterations = 0 is that call"""
    fa, fb = cases[n]
    raw = ctx.descriptor_match(fa[1], fb[1], 10000, RATIO)
    for trials in (0, 1000):
        amd.random_seed(7, 8)
        em = amd.match_features(fa[0], fa[1], fb[0], fb[1], RATIO, trials, EPS, ctx=ctx)
        after = _color(amd)
        amd.random_seed(7, 8)
        gm, gf = amd.match_features_fundamental(fa[0], fa[1], fb[0], fb[1], RATIO, trials, EPS, ctx=ctx)
        assert after == _color(amd)
        assert gm.dtype == em.dtype and np.array_equal(gm, em), (n, trials)
        amd.random_seed(7, 8)
        hm, hf = amd.remove_outliers_fundamental(fa[0], fb[0], raw, trials, EPS_MODEL, EPS)
        assert after == _color(amd)
        _same3((gm, gf, 0), (hm, hf, 0), (n, trials, "host"))
        if trials == 0 or n < 8:
            assert gf is None
        elif n >= 257:
            assert gf is not None
        amd.random_seed(7, 8)
        zm, zf, zi = amd.match_features_fundamental_refined(fa[0], fa[1], fb[0], fb[1], RATIO, trials, EPS, 0, ctx=ctx)
        assert after == _color(amd)
        _same3((zm, zf, zi), (gm, gf, 0), (n, trials, "zero iterations"))


def _pair_sets(amd, cases, nb=61):
    """sets 0 / 1, 2 / 3, 4 / 5: planted cases of 257, 1000 and 7 matches; set 6: 300 rows unrelated to all of them; set 7: empty"""
    if nb == 61:
        feats = [f for n in (257, 1000, 7) for f in cases[n]]
    else:
        feats = [f for n in (257, 1000, 7) for f in planted_case(amd, n, SEEDS[n], nb=nb)]
    rng = np.random.default_rng(99)
    k = np.zeros(300, amd.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 1920, 300), rng.uniform(0, 1080, 300)
    feats.append((k, rng.integers(0, 256, (300, nb), dtype=np.uint8)))
    feats.append((np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, nb), np.uint8)))
    # a repeated pair, a reversed pair, an (a, a) pair, a pair of unrelated sets, a pair with fewer than 8 matches, an empty set on
    # either side
    pairs = [(0, 1), (2, 3), (0, 1), (1, 0), (2, 2), (0, 6), (4, 5), (0, 7), (7, 2)]
    return feats, pairs


def test_pairs_unrefined_equal_match_features_pairs(ctx, amd, cases):
    feats, pairs = _pair_sets(amd, cases)
    amd.random_seed(42, 69)
    exp = ctx.match_features_pairs(feats, pairs, RATIO, 1000, EPS)
    after = _color(amd)
    amd.random_seed(42, 69)
    got = ctx.match_features_fundamental_pairs(feats, pairs, RATIO, 1000, EPS)
    assert after == _color(amd)
    amd.random_seed(42, 69)
    for p, ((a, b), (gm, gf), em) in enumerate(zip(pairs, got, exp)):
        assert gm.dtype == em.dtype and np.array_equal(gm, em), p
        _same3((gm, gf, 0), _host(ctx, amd, feats[a], feats[b], RATIO, 1000, EPS, 0), ("host", p))
    assert after == _color(amd)
    # (the (a, a) pair: equal points give design rows of rank 6, no trial has a model, the zero model keeps every match)
    assert all(got[p][1] is not None for p in (0, 1, 2, 3)) and all(got[p][1] is None for p in (4, 6, 7, 8))
    assert len(got[4][0]) == 1000


@pytest.mark.parametrize("nb,its", [(61, 1), (61, 8), (64, 8)])
def test_pairs_equal_the_loop_of_the_single_call(ctx, amd, cases, nb, its):
    feats, pairs = _pair_sets(amd, cases, nb)
    amd.random_seed(42, 69)
    got = ctx.match_features_fundamental_refined_pairs(feats, pairs, RATIO, 1000, EPS, its)
    after_batch = _color(amd)
    amd.random_seed(42, 69)
    exp = [amd.match_features_fundamental_refined(feats[a][0], feats[a][1], feats[b][0], feats[b][1], RATIO, 1000, EPS, its, ctx=ctx)
           for a, b in pairs]
    assert after_batch == _color(amd)
    assert len(got) == len(pairs)
    for p, (g, e) in enumerate(zip(got, exp)):
        _same3(g, e, (p, pairs[p]))
    assert got[0][1] is not None and got[1][1] is not None and got[3][1] is not None
    assert got[4][1] is None and got[4][2] == 0 and len(got[4][0]) == 1000   # (a, a): no trial has a model
    assert got[6][1] is None and got[6][2] == 0 and len(got[6][0]) == 7
    assert got[7][1] is None and len(got[7][0]) == 0 and got[8][1] is None and len(got[8][0]) == 0
    assert sum(g[2] > 0 for g in got) >= 2                 # (the stage did run: by the host statement, 2 pairs or more accept a fit
                                                           # from each seed this file uses; the repeated pair draws other samples)
    # against the host composite too, from the same seed, and the module-level twin
    amd.random_seed(42, 69)
    for p, (a, b) in enumerate(pairs):
        _same3(got[p], _host(ctx, amd, feats[a], feats[b], RATIO, 1000, EPS, its), ("host", p))
    amd.random_seed(42, 69)
    twin = amd.match_features_fundamental_refined_pairs(feats, pairs[:3], RATIO, 1000, EPS, its, ctx=ctx)
    for g, e in zip(twin, got[:3]):
        _same3(g, e, "twin")


def test_refusals_come_before_the_first_draw(ctx, amd, cases):
    feats, pairs = _pair_sets(amd, cases)
    amd.random_seed(42, 69)
    fresh = _color(amd)
    more = list(feats)
    more[3] = (feats[3][0][:10], feats[3][1])              # more descriptors than keypoints, in the second pair
    calls = [lambda: ctx.match_features_fundamental_pairs(feats, pairs + [(0, 9)], RATIO, 1000, EPS),
             lambda: ctx.match_features_fundamental_refined_pairs(more, pairs, RATIO, 1000, EPS, 8),
             lambda: ctx.match_features_fundamental_guided_pairs(feats, pairs, RATIO, 1000, EPS, -1.0, RATIO),
             lambda: ctx.match_features_fundamental_refined_guided_pairs(feats, pairs, RATIO, 1000, EPS, 8, float("nan"), RATIO),
             lambda: amd.match_features_fundamental_refined(more[2][0], more[2][1], more[3][0], more[3][1], RATIO, 1000, EPS, 8, ctx=ctx)]
    for k, call in enumerate(calls):
        amd.random_seed(42, 69)
        with pytest.raises(amd.AkazeError):
            call()
        assert _color(amd) == fresh, k


@pytest.mark.parametrize("its", [0, 8])
def test_guided_forms(ctx, amd, cases, its):
    """its = 0: the _guided forms (the winner gates); its = 8: the _refined_guided forms (the refined F gates)"""
    feats, pairs = _pair_sets(amd, cases)

    def single(fa, fb, radius, gratio):
        if its == 0:
            return (*amd.match_features_fundamental_guided(fa[0], fa[1], fb[0], fb[1], RATIO, 1000, EPS, radius, gratio, ctx=ctx), 0)
        return amd.match_features_fundamental_refined_guided(fa[0], fa[1], fb[0], fb[1], RATIO, 1000, EPS, its, radius, gratio, ctx=ctx)

    def batch(c, pr, radius, gratio):
        if its == 0:
            return [(*g, 0) for g in c.match_features_fundamental_guided_pairs(feats, pr, RATIO, 1000, EPS, radius, gratio)]
        return c.match_features_fundamental_refined_guided_pairs(feats, pr, RATIO, 1000, EPS, its, radius, gratio)

    def guided(fa, fb, f, radius, gratio):
        return amd.descriptor_match_guided_host(fa[0], fa[1], fb[0], fb[1], f, amd.GUIDED_FUNDAMENTAL, radius, 10000, gratio)
    n_guided = 0
    for radius, gratio in ((3.0, RATIO), (1.0, 0.95)):
        for a, b in ((0, 1), (4, 5), (0, 6)):               # a model, fewer than 8 matches, unrelated sets
            fa, fb = feats[a], feats[b]
            amd.random_seed(5, 6)
            gm, gf, gi = single(fa, fb, radius, gratio)
            after = _color(amd)
            amd.random_seed(5, 6)
            rm, rf, ri = amd.match_features_fundamental_refined(fa[0], fa[1], fb[0], fb[1], RATIO, 1000, EPS, its, ctx=ctx)
            assert after == _color(amd)
            em = rm if rf is None else guided(fa, fb, rf, radius, gratio)   # found = 0: the unrefined list
            _same3((gm, gf, gi), (em, rf, ri), (a, b, radius))
        amd.random_seed(5, 6)
        got = batch(ctx, pairs, radius, gratio)
        after = _color(amd)
        amd.random_seed(5, 6)
        ref = ctx.match_features_fundamental_refined_pairs(feats, pairs, RATIO, 1000, EPS, its)
        assert after == _color(amd)
        for p, ((a, b), g, (rm, rf, ri)) in enumerate(zip(pairs, got, ref)):
            fa, fb = feats[a], feats[b]
            em = rm if rf is None else guided(fa, fb, rf, radius, gratio)
            _same3(g, (em, rf, ri), (p, radius))
            n_guided += rf is not None
    assert n_guided >= 6
    if its:
        assert sum(g[2] > 0 for g in got) >= 2


def test_second_context_beside_extraction(ctx, amd, cases):
    import torch
    feats, pairs = _pair_sets(amd, cases)
    other = amd.Context(0, torch.cuda.Stream().cuda_stream)
    try:
        amd.random_seed(3, 4)
        exp = ctx.match_features_fundamental_refined_pairs(feats, pairs, RATIO, 1000, EPS, 8)
        amd.random_seed(3, 4)
        exp_g = ctx.match_features_fundamental_refined_guided_pairs(feats, pairs, RATIO, 1000, EPS, 8, 3.0, RATIO)
        frames = torch.from_numpy(np.stack([amd.synth_frame(1920, 1080, 40 + i) for i in range(4)])).cuda()
        job = ctx.extract_begin(frames, keep_all_planes=False)
        amd.random_seed(3, 4)
        got = other.match_features_fundamental_refined_pairs(feats, pairs, RATIO, 1000, EPS, 8)
        amd.random_seed(3, 4)
        got_g = other.match_features_fundamental_refined_guided_pairs(feats, pairs, RATIO, 1000, EPS, 8, 3.0, RATIO)
        res = job.finish()
        assert res.counts(0)[1] > 0
        for p, (g, e) in enumerate(zip(got, exp)):
            _same3(g, e, p)
        for p, (g, e) in enumerate(zip(got_g, exp_g)):
            _same3(g, e, ("guided", p))
        assert sum(g[2] > 0 for g in got) >= 2
    finally:
        other.close()
