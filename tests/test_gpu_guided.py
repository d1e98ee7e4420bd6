"""Guided matching on the GPU: the device scan equals the host statement bit for bit (both kinds, every radius, ragged
sizes, 21 .. 64-byte rows, several chunks), the pairs call equals the loop, the composite with the homography RANSAC
equals its two stages called one after the other, the guided list contains every match the homography call keeps and
is longer on repeated structure, and all of it holds beside an extraction in flight on another context."""
import numpy as np
import pytest

from test_gpu_match_pairs import _color, _feat, _pair_list
from test_gpu_homography import _descriptor_case, _hbits
from test_homography_host import synthetic_case

pytestmark = pytest.mark.gpu

def _translation(dx, dy):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]], np.float32)


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]], np.float32)


def _shift_of(ctx, fa, fb):
    """The whole-pixel displacement between two shifted frames: the median over the blind matches."""
    m = ctx.descriptor_match(fa[1], fb[1], 10000, 0.86)
    assert len(m) > 50
    dx = np.median(fb[0]["x"][m["index_1"]] - fa[0]["x"][m["index_0"]])
    dy = np.median(fb[0]["y"][m["index_1"]] - fa[0]["y"][m["index_0"]])
    return float(np.rint(dx)), float(np.rint(dy))


def _models(dx, dy):
    """kind -> model of a pure image shift: the translation H, and F = [t]x with t = (dx, dy, 0), whose epipolar lines run
    along the shift (p1 = p0 + s t satisfies p1^T [t]x p0 = 0)."""
    return {0: _translation(dx, dy), 1: _skew((dx, dy, 0.0))}


def _both(ctx, amd, fa, fb, model, kind, radius, thr=10000, ratio=0.86):
    got = amd.descriptor_match_guided(fa[0], fa[1], fb[0], fb[1], model, kind, radius, thr, ratio, ctx=ctx)
    exp = amd.descriptor_match_guided_host(fa[0], fa[1], fb[0], fb[1], model, kind, radius, thr, ratio)
    assert got.dtype == amd.MATCH_DTYPE and np.array_equal(got, exp), (kind, radius, thr, ratio, len(got), len(exp))
    return got


@pytest.fixture(scope="module")
def six(ctx, amd):
    sizes = [(960, 540), (1280, 720)]
    return [_feat(ctx, amd, *sizes[i % 2], 21, shift=(7 * i, 3 * i)) for i in range(6)]


@pytest.fixture(scope="module")
def shifted(ctx, amd):
    fa, fb = _feat(ctx, amd, 960, 540, 21), _feat(ctx, amd, 960, 540, 21, shift=(7, 3))
    return fa, fb, _shift_of(ctx, fa, fb)


def test_device_equals_host(ctx, amd, shifted):
    fa, fb, (dx, dy) = shifted
    assert (abs(dx), abs(dy)) == (7.0, 3.0)
    lens = {}
    for kind, model in _models(dx, dy).items():
        for radius in (0.0, 0.5, 3.0, 50.0, 1e18):
            for ratio in (0.6, 0.86):
                for thr in (10000, 100):
                    lens[kind, radius, ratio, thr] = len(_both(ctx, amd, fa, fb, model, kind, radius, thr, ratio))
            assert (lens[kind, radius, 0.86, 10000] == 0) == (radius == 0.0), (kind, radius)
        # a wider gate only adds candidates; everything passing is the blind scan
        blind = ctx.descriptor_match(fa[1], fb[1], 10000, 0.86)
        assert np.array_equal(amd.descriptor_match_guided(*fa, *fb, model, kind, 1e18, 10000, 0.86, ctx=ctx), blind)
        assert lens[kind, 3.0, 0.86, 10000] > len(blind)  # the feature at work: the gate lets the ratio test pass more


def test_descriptor_channels(ctx, amd):
    for ch in (1, 2, 3):
        fa = _feat(ctx, amd, 960, 540, 4, descriptor_channels=ch)
        fb = _feat(ctx, amd, 960, 540, 4, shift=(5, 2), descriptor_channels=ch)
        assert fa[1].shape[1] == {1: 21, 2: 41, 3: 61}[ch]
        dx, dy = _shift_of(ctx, fa, fb)
        for kind, model in _models(dx, dy).items():
            for radius in (3.0, 1e18):
                assert len(_both(ctx, amd, fa, fb, model, kind, radius)) > 0


def test_64_byte_rows_compare_every_byte(ctx, amd):
    """Train rows come in pairs at the same place that differ only in bytes 61..63; the query carries the bytes of the
    SECOND copy: comparing 61 bytes would see two equal candidates and keep nothing."""
    rng = np.random.default_rng(5)
    n = 700
    d0 = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    first = d0.copy()
    first[:, 61:] ^= 0x5A
    d1 = np.concatenate([first, d0])
    k0 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k0["x"], k0["y"] = rng.uniform(0, 800, n), rng.uniform(0, 600, n)
    k1 = np.concatenate([k0, k0])
    k1["x"] += 4.0
    k1["y"] -= 2.0
    for kind, model in _models(4.0, -2.0).items():
        for radius in (0.5, 3.0, 1e18):
            got = _both(ctx, amd, (k0, d0), (k1, d1), model, kind, radius, ratio=1.5)
            assert len(got) == n and np.array_equal(got["index_1"], np.arange(n, 2 * n)) and np.all(got["distance"] == 0)
            # cut to 61 bytes the two copies tie at distance 0, and min < second ratio^2 fails at any ratio: nothing is kept
            cut = _both(ctx, amd, (k0, d0[:, :61]), (k1, d1[:, :61]), model, kind, radius, ratio=1.5)
            assert len(cut) == 0


def test_ragged_sizes(ctx, amd, shifted):
    fa, fb, (dx, dy) = shifted
    na, nb = len(fa[1]), len(fb[1])
    assert na > 300 and nb > 300
    for kind, model in _models(dx, dy).items():
        for n0, n1 in ((1, 1), (33, 1), (1, 777), (257, 129), (100, 0), (0, 100), (0, 0), (513, 1001), (na, nb - 1)):
            # (keypoints stay whole: more keypoints than descriptors, and only the first n are read)
            a, b = (fa[0], fa[1][:n0]), (fb[0], fb[1][:n1])
            for radius in (3.0, 1e18):
                got = _both(ctx, amd, a, b, model, kind, radius)
                assert n0 and n1 or len(got) == 0


def test_several_chunks(ctx, amd):
    """The launch honours Context.debug_set_match_chunks: a train set cut into 5 and 64 chunks gives the list of one."""
    fa, fb = _feat(ctx, amd, 1920, 1080, 21), _feat(ctx, amd, 1920, 1080, 21, shift=(7, 3))
    dx, dy = _shift_of(ctx, fa, fb)
    assert len(fb[1]) > 3 * 256  # (the forced count is capped at the set's LDS tiles of 256 rows: at least 3 chunks below)
    try:
        for chunks in (5, 64, 3):
            ctx.debug_set_match_chunks(chunks, 0)
            for kind, model in _models(dx, dy).items():
                for radius in (3.0, 50.0, 1e18):
                    _both(ctx, amd, fa, fb, model, kind, radius)
                    _both(ctx, amd, (fa[0], fa[1][:300]), fb, model, kind, radius)  # (the single-workgroup compaction)
    finally:
        ctx.debug_set_match_chunks(0, 0)


def _pair_models(pairs, kind):
    """A model of its own for every pair: the shift between frames a and b of `six`, either sign (the test compares two
    paths, it does not need the true one), and a little rotation that grows with the pair's number."""
    out = []
    for p, (a, b) in enumerate(pairs):
        dx, dy = 7.0 * (b - a), 3.0 * (b - a)
        if kind == 0:
            h = _translation(dx, dy)
            h[0, 1], h[1, 0] = 1e-4 * p, -1e-4 * p
            out.append(h)
        else:
            out.append(_skew((dx if a != b else 1.0, dy, 1e-3 * p)))
    return np.stack(out)


def test_pairs_equal_loop(ctx, amd, six):
    empty = (np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, 61), np.uint8))
    one = (six[1][0], six[1][1][:1])
    edge_feats = list(six[:3]) + [empty, one]
    edge_pairs = [(0, 1), (3, 1), (1, 3), (3, 3), (2, 2), (1, 0), (4, 2), (2, 4), (0, 1), (4, 4), (2, 0)]
    for feats, pairs in ((six, _pair_list()), (edge_feats, edge_pairs)):
        for kind in (0, 1):
            models = _pair_models(pairs, kind)
            for radius, thr, ratio in ((3.0, 10000, 0.86), (50.0, 100, 0.6), (1e18, 10000, 0.86)):
                got = ctx.descriptor_match_guided_pairs(feats, pairs, models, kind, radius, thr, ratio)
                assert len(got) == len(pairs)
                for p, (a, b) in enumerate(pairs):
                    exp = amd.descriptor_match_guided(*feats[a], *feats[b], models[p], kind, radius, thr, ratio, ctx=ctx)
                    assert np.array_equal(got[p], exp), (kind, radius, p, (a, b), len(got[p]), len(exp))
                assert sum(len(g) for g in got) > 0
    # a few pairs against the host statement as well
    pairs = [(0, 2), (3, 1), (2, 2)]
    for kind in (0, 1):
        models = _pair_models(pairs, kind)
        got = ctx.descriptor_match_guided_pairs(six, pairs, models, kind, 3.0)
        for p, (a, b) in enumerate(pairs):
            assert np.array_equal(got[p], amd.descriptor_match_guided_host(*six[a], *six[b], models[p], kind, 3.0))
    assert ctx.descriptor_match_guided_pairs(six, [], np.zeros((0, 9)), 0, 3.0) == []


def _composition(ctx, amd, feats, pairs, ratio, trials, eps, g_radius, g_ratio, seed):
    """The homography pairs call, then descriptor_match_guided_pairs over the pairs it found a model for."""
    amd.random_seed(*seed)
    base = ctx.match_features_homography_pairs(feats, pairs, ratio, trials, eps)
    after = _color(amd)
    found = [p for p, (_, h) in enumerate(base) if h is not None]
    guided = ctx.descriptor_match_guided_pairs(feats, [pairs[p] for p in found], np.stack([base[p][1] for p in found]) if found
                                               else np.zeros((0, 9)), amd.GUIDED_HOMOGRAPHY, g_radius, 10000, g_ratio)
    exp = list(base)
    for p, g in zip(found, guided):
        exp[p] = (g, base[p][1])
    return base, exp, after


def _composite_equals_composition(ctx, amd, feats, pairs, ratio, trials, eps, g_radius, g_ratio, seed=(42, 69)):
    amd.random_seed(*seed)
    got = ctx.match_features_homography_guided_pairs(feats, pairs, ratio, trials, eps, g_radius, g_ratio)
    after = _color(amd)
    base, exp, after_exp = _composition(ctx, amd, feats, pairs, ratio, trials, eps, g_radius, g_ratio, seed)
    assert after == after_exp and len(got) == len(exp) == len(pairs)
    for p, ((gm, gh), (em, eh)) in enumerate(zip(got, exp)):
        assert (gh is None) == (eh is None), p
        assert gh is None or np.array_equal(_hbits(gh), _hbits(eh)), p
        assert np.array_equal(gm, em), (p, pairs[p], len(gm), len(em))
        if gh is None:
            assert np.array_equal(gm, base[p][0]), p  # without a winner: the homography call's list
    return got, base


@pytest.mark.parametrize("trials", [0, 8, 1000])
def test_composite_equals_composition(ctx, amd, six, trials):
    empty = (np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, 61), np.uint8))
    few = (six[0][0][:3], six[0][1][:3])  # fewer than 4 matches: no model
    feats = list(six) + [empty, few]
    pairs = _pair_list() + [(6, 1), (1, 6), (7, 0), (0, 7), (6, 6)]
    n_found = 0
    for eps, ratio, g_radius, g_ratio in ((3.0, 0.86, 3.0, 0.86), (0.5, 0.6, 10.0, 0.9)):
        got, _ = _composite_equals_composition(ctx, amd, feats, pairs, ratio, trials, eps, g_radius, g_ratio)
        n_found += sum(h is not None for _, h in got)
    assert (n_found > 0) == (trials > 0)
    # the one-pair call is the pairs call with one pair
    amd.random_seed(5, 6)
    gm, gh = amd.match_features_homography_guided(*six[0], *six[2], 0.86, trials, 3.0, 3.0, 0.86, ctx=ctx)
    amd.random_seed(5, 6)
    (em, eh), = ctx.match_features_homography_guided_pairs(six, [(0, 2)], 0.86, trials, 3.0, 3.0, 0.86)
    assert np.array_equal(gm, em) and (gh is None) == (eh is None) and (gh is None or np.array_equal(_hbits(gh), _hbits(eh)))


def test_composite_64_byte_rows(ctx, amd):
    rng = np.random.default_rng(8)
    n = 600
    base = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    d1 = np.concatenate([base[rng.permutation(n)], base])
    d1[:n, 61:] ^= 0x5A
    k0 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k0["x"], k0["y"] = rng.uniform(0, 800, n), rng.uniform(0, 600, n)
    k1 = np.zeros(2 * n, amd.KEYPOINT_DTYPE)
    k1["x"] = np.concatenate([rng.uniform(0, 800, n), k0["x"] + 3.0])
    k1["y"] = np.concatenate([rng.uniform(0, 600, n), k0["y"] + 1.0])
    got, _ = _composite_equals_composition(ctx, amd, [(k0, base), (k1, d1)], [(0, 1), (1, 0), (0, 0)], 0.95, 500, 5.0, 5.0, 0.95)
    assert got[0][1] is not None and len(got[0][0]) > 0


def _assert_superset(base, got):
    """Every match the homography call keeps is in the guided list with the same index_1 and distance.  Exact, not
    empirical, when guided_radius = ransac_epsilon_inliers and guided_lowes_ratio = lowes_ratio: a kept match passes the
    same homography_inlier, it stays the lowest-index minimum of a subset that contains it, and the subset's second
    distance can only be larger."""
    (bm, bh), (gm, gh) = base, got
    assert (bh is None) == (gh is None)
    if bh is None:  # no model: the homography call's list, unchanged
        assert np.array_equal(gm, bm)
        return False
    at = np.searchsorted(gm["index_0"], bm["index_0"])
    assert np.all(at < len(gm)) and np.array_equal(gm[at], bm), (len(bm), len(gm))
    return True


def test_superset_of_the_homography_list(ctx, amd, six):
    # (frames 0, 2, 4 and 1, 3, 5 of `six` have one size each and share a scene; (0, 1) and (1, 0) do not and find no model)
    pairs = [(0, 1), (1, 0), (2, 4), (5, 3), (0, 2), (3, 1)]
    for eps, ratio in ((3.0, 0.86), (1.0, 0.7)):
        got, base = _composite_equals_composition(ctx, amd, six, pairs, ratio, 1000, eps, eps, ratio)
        assert sum(_assert_superset(base[p], got[p]) for p in range(len(pairs))) >= 4
    for seed in range(4):
        k0, d0, k1, d1, m, inl = _descriptor_case(amd, seed)
        got, base = _composite_equals_composition(ctx, amd, [(k0, d0), (k1, d1)], [(0, 1)], 0.86, 1000, 2.0, 2.0, 0.86)
        assert _assert_superset(base[0], got[0])
        assert np.array_equal(base[0][0], m[inl])


def repetitive_case(amd, seed=0, n_unique=500, groups=60, copies=8):
    """Repeated structure, as a facade of identical windows gives: n_unique points with descriptors of their own and
    groups x copies points whose descriptors are one pattern per group with one random bit flipped per copy, spread over
    a 1920 x 1080 frame; image 1 is image 0 under H_true of synthetic_case(seed) with the train rows permuted and twelve
    more bits flipped per row.
    How it was chosen: on the CPU, with akz_descriptor_match_guided_host and the oracle.  The blind scan at ratio 0.86
    keeps the 500 unique rows and none of the 480 repeated ones (best 12 bits to the true partner, second at most 14 bits to a
    sibling: 12 >= 14 x 0.86^2 = 10.4); the guided scan with H_true and a 3-pixel disc sees the partner alone and keeps all 980
    (seed 0: 500 blind, 980 guided).  The numbers are asserted on the host path below before the GPU is asked."""
    rng = np.random.default_rng(7000 + seed)
    h = synthetic_case(amd, seed)[4]
    n = n_unique + groups * copies
    p0 = np.zeros((0, 2))
    while len(p0) < n:
        c = rng.uniform([0, 0], [1920, 1080], (n, 2))
        p0 = np.r_[p0, c[c @ h[2, :2] + 1.0 > 0.2]]
    p0 = p0[:n].astype(np.float32).astype(np.float64)
    q = np.c_[p0, np.ones(n)] @ h.T
    p1 = (q[:, :2] / q[:, 2:]).astype(np.float32)
    d0 = rng.integers(0, 256, (n, 61), dtype=np.uint8)
    pattern = rng.integers(0, 256, (groups, 61), dtype=np.uint8)
    d0[n_unique:] = np.repeat(pattern, copies, axis=0)

    def flip(d, bits):
        d = d.copy()
        for r in range(len(d)):
            for b in rng.choice(61 * 8, bits, replace=False):
                d[r, b // 8] ^= np.uint8(1 << (b % 8))
        return d

    d0[n_unique:] = flip(d0[n_unique:], 1)
    perm = rng.permutation(n)
    k0 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k1 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k0["x"], k0["y"] = p0[:, 0], p0[:, 1]
    k1["x"][perm], k1["y"][perm] = p1[:, 0], p1[:, 1]
    d1 = np.zeros_like(d0)
    d1[perm] = flip(d0, 12)
    return (k0, d0), (k1, d1), h, perm, n_unique


def test_guided_list_is_longer_on_repeated_structure(ctx, amd, ref):
    fa, fb, h_true, perm, n_unique = repetitive_case(amd)
    n = len(perm)
    blind = ref.descriptor_match(fa[1], fb[1], 10000, 0.86)
    host = amd.descriptor_match_guided_host(*fa, *fb, h_true, amd.GUIDED_HOMOGRAPHY, 3.0, 10000, 0.86)
    assert len(blind) == n_unique and np.array_equal(blind["index_0"], np.arange(n_unique))
    assert len(host) == n and np.array_equal(host["index_1"], perm)
    amd.random_seed(42, 69)
    base, _ = ctx.match_features_homography_pairs([fa, fb], [(0, 1)], 0.86, 1000, 3.0)[0]
    amd.random_seed(42, 69)
    got, h = amd.match_features_homography_guided(*fa, *fb, 0.86, 1000, 3.0, 3.0, 0.86, ctx=ctx)
    assert h is not None and len(base) <= n_unique
    assert len(got) > len(base)                                   # strictly longer ...
    assert len(got) >= n - 20 and np.array_equal(got["index_1"], perm[got["index_0"]])  # ... and right: the true partners
    at = np.searchsorted(got["index_0"], base["index_0"])
    assert np.array_equal(got[at], base)


def test_second_context_beside_extraction(ctx, amd, six):
    import torch
    other = amd.Context(0, torch.cuda.Stream().cuda_stream)
    try:
        pairs = [(0, 2), (2, 4), (1, 3), (5, 1), (0, 1)]
        models = _pair_models(pairs, 1)
        exp_f = ctx.descriptor_match_guided_pairs(six, pairs, models, 1, 3.0)
        amd.random_seed(3, 4)
        exp_h = ctx.match_features_homography_guided_pairs(six, pairs, 0.86, 1000, 3.0, 3.0, 0.86)
        frames = torch.from_numpy(np.stack([amd.synth_frame(1920, 1080, 40 + i) for i in range(4)])).cuda()
        job = ctx.extract_begin(frames, keep_all_planes=False)
        got_f = other.descriptor_match_guided_pairs(six, pairs, models, 1, 3.0)
        amd.random_seed(3, 4)
        got_h = other.match_features_homography_guided_pairs(six, pairs, 0.86, 1000, 3.0, 3.0, 0.86)
        res = job.finish()
        assert res.counts(0)[1] > 0
        for g, e in zip(got_f, exp_f):
            assert np.array_equal(g, e)
        for (gm, gh), (em, eh) in zip(got_h, exp_h):
            assert np.array_equal(gm, em) and (gh is None) == (eh is None)
            assert gh is None or np.array_equal(_hbits(gh), _hbits(eh))
        assert sum(h is not None for _, h in got_h) >= 4
    finally:
        other.close()
