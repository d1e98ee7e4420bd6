"""The refit stage on the GPU (akz_match_features_homography_refined and its pairs / guided forms): the device result equals
the host composite descriptor_match -> remove_outliers_homography -> refine_homography on the raw list bit for bit (list, H,
found, accepted fits, the random source's state), refine_iterations = 0 is the unrefined call, the pairs call is the loop of
the single call, the guided forms gate with the refined H, a real warp holds, and a second context runs it beside an
extraction.  Small planted-descriptor sets throughout: descriptor_match returns exactly the planted matches."""
import numpy as np
import pytest

from test_gpu_homography import _hbits, inlier_rule, warp_case
from test_gpu_match_pairs import _color
from test_homography_host import _apply
from test_homography_refit_host import _h_true, _points

pytestmark = pytest.mark.gpu

SIZES = [3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 3001]
EPS = 3.0
RATIO = 0.86


def planted_case(amd, n, seed, nb=61, sigma=0.7, outliers=0.35):
    """n keypoints per image, keypoint i of image 0 matching keypoint perm[i] of image 1 through equal random descriptors:
    inliers H_true p0 + N(0, sigma), a share of outliers displaced at least 50 px.  Returns ((k0, d0), (k1, d1), H_true)."""
    rng = np.random.default_rng(seed)
    h = _h_true(rng)
    p0 = _points(rng, h, n)
    out = rng.uniform(size=n) < outliers
    p1 = _apply(h, p0) + rng.normal(0, sigma, (n, 2)) * (~out)[:, None]
    ang, dist = rng.uniform(0, 2 * np.pi, n), rng.uniform(50, 400, n)
    p1[out] += (np.c_[np.cos(ang), np.sin(ang)] * dist[:, None])[out]
    perm = rng.permutation(n)
    k0 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k1 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k0["x"], k0["y"] = p0[:, 0], p0[:, 1]
    k1["x"][perm], k1["y"][perm] = p1[:, 0], p1[:, 1]
    d0 = rng.integers(0, 256, (n, nb), dtype=np.uint8)
    d1 = np.zeros_like(d0)
    d1[perm] = d0
    return (k0, d0), (k1, d1), h


@pytest.fixture(scope="module")
def cases(amd):
    """one planted case per size (built once, left unchanged)"""
    return {n: planted_case(amd, n, 500 + n) for n in SIZES}


def _host(ctx, amd, fa, fb, ratio, trials, eps, its):
    """the host composite -> (list, H or None, accepted fits)"""
    raw = ctx.descriptor_match(fa[1], fb[1], 10000, ratio)
    kept, h = amd.remove_outliers_homography(fa[0], fb[0], raw, trials, amd.HOMOGRAPHY_EPSILON_MODEL, eps)
    if h is None or its == 0:
        return kept, h, 0
    return amd.refine_homography(fa[0], fb[0], raw, h, eps, its)


def _same3(got, exp, what):
    (gm, gh, gi), (em, eh, ei) = got, exp
    assert gm.dtype == em.dtype and np.array_equal(gm, em), (what, len(gm), len(em))
    assert (gh is None) == (eh is None), what
    if gh is not None:
        assert np.array_equal(_hbits(gh), _hbits(eh)), (what, gh, eh)
    assert gi == ei, (what, gi, ei)


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host_composite(ctx, amd, cases, n):
    fa, fb, _ = cases[n]
    raw = ctx.descriptor_match(fa[1], fb[1], 10000, RATIO)
    assert len(raw) == n                                   # the planted matches, all of them
    fitted = False
    for trials in (0, 1, 1000):
        for its in (1, 2, 8):
            amd.random_seed(42, 69)
            got = amd.match_features_homography_refined(fa[0], fa[1], fb[0], fb[1], RATIO, trials, EPS, its, ctx=ctx)
            after_dev = _color(amd)
            amd.random_seed(42, 69)
            exp = _host(ctx, amd, fa, fb, RATIO, trials, EPS, its)
            after_host = _color(amd)
            _same3(got, exp, (n, trials, its))
            assert after_dev == after_host, (n, trials, its)
            assert got[2] <= its
            if trials == 0 or n < 4:
                assert got[1] is None and got[2] == 0 and np.array_equal(got[0], raw)
            fitted |= got[2] > 0
    if n >= 63:
        assert fitted, n                                   # (the stage did run a fit that was accepted)


@pytest.mark.parametrize("n", [5, 257, 1000])
def test_zero_iterations_is_the_unrefined_call(ctx, amd, cases, n):
    fa, fb, _ = cases[n]
    for trials in (0, 1000):
        amd.random_seed(7, 8)
        gm, gh, gi = amd.match_features_homography_refined(fa[0], fa[1], fb[0], fb[1], RATIO, trials, EPS, 0, ctx=ctx)
        after = _color(amd)
        amd.random_seed(7, 8)
        em, eh = amd.match_features_homography(fa[0], fa[1], fb[0], fb[1], RATIO, trials, EPS, ctx=ctx)
        assert after == _color(amd)
        _same3((gm, gh, gi), (em, eh, 0), (n, trials))


def _pair_sets(amd, cases, nb=61):
    """sets 0 / 1, 2 / 3, 4 / 5: planted cases of 257, 1000 and 3 matches; set 6: unrelated to all of them"""
    if nb == 61:
        feats = [f for n in (257, 1000, 3) for f in cases[n][:2]]
    else:
        feats = [f for n in (257, 1000, 3) for f in planted_case(amd, n, 900 + n, nb=nb)[:2]]
    rng = np.random.default_rng(99)
    k = np.zeros(300, amd.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 1920, 300), rng.uniform(0, 1080, 300)
    feats.append((k, rng.integers(0, 256, (300, nb), dtype=np.uint8)))
    # a repeated pair, a reversed pair, an (a, a) pair, a pair of unrelated sets, a pair with fewer than 4 matches
    pairs = [(0, 1), (2, 3), (0, 1), (1, 0), (2, 2), (0, 6), (4, 5)]
    return feats, pairs


@pytest.mark.parametrize("nb,its", [(61, 1), (61, 8), (64, 8)])
def test_pairs_equal_the_loop_of_the_single_call(ctx, amd, cases, nb, its):
    feats, pairs = _pair_sets(amd, cases, nb)
    amd.random_seed(42, 69)
    got = ctx.match_features_homography_refined_pairs(feats, pairs, RATIO, 1000, EPS, its)
    after_batch = _color(amd)
    amd.random_seed(42, 69)
    exp = [amd.match_features_homography_refined(feats[a][0], feats[a][1], feats[b][0], feats[b][1], RATIO, 1000, EPS, its, ctx=ctx)
           for a, b in pairs]
    assert after_batch == _color(amd)
    assert len(got) == len(pairs)
    for p, (g, e) in enumerate(zip(got, exp)):
        _same3(g, e, (p, pairs[p]))
    assert got[0][1] is not None and got[1][1] is not None and got[3][1] is not None and got[4][1] is not None
    assert got[6][1] is None and got[6][2] == 0 and len(got[6][0]) == 3
    assert sum(g[2] > 0 for g in got) >= 3
    # against the host composite too, from the same seed, and the module-level twin
    amd.random_seed(42, 69)
    for p, (a, b) in enumerate(pairs):
        _same3(got[p], _host(ctx, amd, feats[a], feats[b], RATIO, 1000, EPS, its), ("host", p))
    amd.random_seed(42, 69)
    twin = amd.match_features_homography_refined_pairs(feats, pairs[:3], RATIO, 1000, EPS, its, ctx=ctx)
    for g, e in zip(twin, got[:3]):
        _same3(g, e, "twin")


def _contains(big, small):
    key = lambda m: set(zip(m["index_0"].tolist(), m["index_1"].tolist(), m["distance"].tolist()))
    return key(small) <= key(big)


@pytest.mark.parametrize("its", [1, 8])
def test_refined_guided_is_the_refined_call_then_the_guided_scan(ctx, amd, cases, its):
    feats, pairs = _pair_sets(amd, cases)
    for radius, gratio in ((EPS, RATIO), (1.5, 0.95)):
        # the single call
        for a, b in ((0, 1), (2, 3), (4, 5), (0, 6)):
            fa, fb = feats[a], feats[b]
            amd.random_seed(5, 6)
            gm, gh, gi = amd.match_features_homography_refined_guided(fa[0], fa[1], fb[0], fb[1], RATIO, 1000, EPS, its, radius, gratio,
                                                                      ctx=ctx)
            after = _color(amd)
            amd.random_seed(5, 6)
            rm, rh, ri = amd.match_features_homography_refined(fa[0], fa[1], fb[0], fb[1], RATIO, 1000, EPS, its, ctx=ctx)
            assert after == _color(amd)
            em = rm if rh is None else amd.descriptor_match_guided(fa[0], fa[1], fb[0], fb[1], rh, amd.GUIDED_HOMOGRAPHY, radius, 10000,
                                                                   gratio, ctx=ctx)
            _same3((gm, gh, gi), (em, rh, ri), (a, b, radius))
            if radius == EPS and gratio == RATIO:
                assert _contains(gm, rm), (a, b)
        # the pairs call
        amd.random_seed(5, 6)
        got = ctx.match_features_homography_refined_guided_pairs(feats, pairs, RATIO, 1000, EPS, its, radius, gratio)
        after = _color(amd)
        amd.random_seed(5, 6)
        ref = ctx.match_features_homography_refined_pairs(feats, pairs, RATIO, 1000, EPS, its)
        assert after == _color(amd)
        for p, ((a, b), g, (rm, rh, ri)) in enumerate(zip(pairs, got, ref)):
            fa, fb = feats[a], feats[b]
            em = rm if rh is None else amd.descriptor_match_guided(fa[0], fa[1], fb[0], fb[1], rh, amd.GUIDED_HOMOGRAPHY, radius, 10000,
                                                                   gratio, ctx=ctx)
            _same3(g, (em, rh, ri), (p, radius))
            if radius == EPS and gratio == RATIO:
                assert _contains(g[0], rm), p
        amd.random_seed(5, 6)
        twin = amd.match_features_homography_refined_guided_pairs(feats, pairs[:2], RATIO, 1000, EPS, its, radius, gratio, ctx=ctx)
        for g, e in zip(twin, got[:2]):
            _same3(g, e, "twin")


def test_real_warp(ctx, amd):
    import torch
    f0, f1, h_true = warp_case(amd)
    res = [ctx.extract_features(f, keep_all_planes=False) for f in (f0, f1)]
    fa, fb = [(r.keypoints(), r.descriptors()) for r in res]
    raw = ctx.descriptor_match(fa[1], fb[1], 10000, RATIO)
    amd.random_seed(42, 69)
    um, uh = amd.match_features_homography(fa[0], fa[1], fb[0], fb[1], RATIO, 1000, EPS, ctx=ctx)
    amd.random_seed(42, 69)
    got = amd.match_features_homography_refined(fa[0], fa[1], fb[0], fb[1], RATIO, 1000, EPS, 8, ctx=ctx)
    amd.random_seed(42, 69)
    _same3(got, _host(ctx, amd, fa, fb, RATIO, 1000, EPS, 8), "warp")
    gm, gh, gi = got
    assert uh is not None and gh is not None
    assert len(gm) >= len(um)
    assert np.array_equal(gm, raw[inlier_rule(gh, fa[0], fb[0], raw, EPS)])
    g = np.stack(np.meshgrid(np.linspace(0, 1280, 9), np.linspace(0, 720, 9)), -1).reshape(-1, 2)
    rms = lambda h: float(np.sqrt(((_apply(h, g) - _apply(h_true, g)) ** 2).sum(axis=1).mean()))
    print("raw", len(raw), "unrefined kept", len(um), "grid rms", rms(uh), "refined kept", len(gm), "grid rms", rms(gh), "fits", gi)
    torch.cuda.synchronize()


def test_second_context_beside_extraction(ctx, amd, cases):
    import torch
    feats, pairs = _pair_sets(amd, cases)
    other = amd.Context(0, torch.cuda.Stream().cuda_stream)
    try:
        amd.random_seed(3, 4)
        exp = ctx.match_features_homography_refined_pairs(feats, pairs, RATIO, 1000, EPS, 8)
        amd.random_seed(3, 4)
        exp_g = ctx.match_features_homography_refined_guided_pairs(feats, pairs, RATIO, 1000, EPS, 8, EPS, RATIO)
        frames = torch.from_numpy(np.stack([amd.synth_frame(1920, 1080, 40 + i) for i in range(4)])).cuda()
        job = ctx.extract_begin(frames, keep_all_planes=False)
        amd.random_seed(3, 4)
        got = other.match_features_homography_refined_pairs(feats, pairs, RATIO, 1000, EPS, 8)
        amd.random_seed(3, 4)
        got_g = other.match_features_homography_refined_guided_pairs(feats, pairs, RATIO, 1000, EPS, 8, EPS, RATIO)
        res = job.finish()
        assert res.counts(0)[1] > 0
        for p, (g, e) in enumerate(zip(got, exp)):
            _same3(g, e, p)
        for p, (g, e) in enumerate(zip(got_g, exp_g)):
            _same3(g, e, ("guided", p))
        assert sum(g[2] > 0 for g in got) >= 3
    finally:
        other.close()
