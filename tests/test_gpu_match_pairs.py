"""akz_match_features_pairs on the GPU: every pair's list equals the loop of match_features over the pairs in order from
the same random state (and leaves the source where that loop does), equals the oracle, holds at the edges (empty sets,
pairs below 8 matches, rank-deficient samples, 21 / 41 / 61 / 64-byte rows), at scale, and beside an extraction in
flight on another context."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _color(amd):
    import ctypes as C
    rgb = (C.c_uint8 * 3)()
    assert amd.lib().akz_random_color(rgb) == 0
    return bytes(rgb)


def _feat(ctx, amd, w, h, idx, shift=(0, 0), **cfg):
    r = ctx.extract_features(amd.synth_frame(w, h, idx, shift=shift), amd.Config(**cfg) if cfg else None,
                             keep_all_planes=False)
    return r.keypoints(), r.descriptors()


def _loop(ctx, amd, feats, pairs, ratio, trials, eps):
    return [amd.match_features(feats[a][0], feats[a][1], feats[b][0], feats[b][1], ratio, trials, eps, ctx=ctx)
            for a, b in pairs]


def _same_as_loop(ctx, amd, feats, pairs, ratio, trials, eps, seed=(42, 69)):
    amd.random_seed(*seed)
    got = ctx.match_features_pairs(feats, pairs, ratio, trials, eps)
    after_batch = _color(amd)
    amd.random_seed(*seed)
    exp = _loop(ctx, amd, feats, pairs, ratio, trials, eps)
    after_loop = _color(amd)
    assert len(got) == len(exp) == len(pairs)
    for p, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == amd.MATCH_DTYPE and np.array_equal(g, e), (p, pairs[p], len(g), len(e), trials, eps, ratio)
    assert after_batch == after_loop, (trials, eps, ratio)
    return got


@pytest.fixture(scope="module")
def six(ctx, amd):
    sizes = [(960, 540), (1280, 720)]
    return [_feat(ctx, amd, *sizes[i % 2], 21, shift=(7 * i, 3 * i)) for i in range(6)]


def _pair_list():
    pairs = list(itertools.permutations(range(6), 2))
    return pairs + [(2, 2), (0, 0), (3, 1), (1, 3), (0, 1), (0, 1)]


@pytest.mark.parametrize("trials", [0, 1, 8, 997, 1000, 4000])
def test_batch_equals_loop(ctx, amd, six, trials):
    pairs = _pair_list()
    drew = False
    for eps in (0.0, 0.5, 3.0, 10.0):
        for ratio in (0.6, 0.86):
            got = _same_as_loop(ctx, amd, six, pairs, ratio, trials, eps)
            drew |= any(len(g) >= 8 for g in got)
    assert drew


def test_batch_equals_oracle(ctx, amd, ref):
    frames = [amd.synth_frame(960, 540, 11, shift=(9 * i, 4 * i)) for i in range(3)]
    res = [ctx.extract_features(f, keep_all_planes=False) for f in frames]
    orc = [ref.extract(f) for f in frames]
    feats = [(r.keypoints(), r.descriptors()) for r in res]
    pairs = [(0, 1), (1, 2), (2, 0), (1, 1), (0, 2)]
    amd.random_seed(42, 69)
    got = ctx.match_features_pairs(feats, pairs, 0.86, 1000, 3.0)
    ref.random_seed(42, 69)
    for p, (a, b) in enumerate(pairs):
        raw = ref.descriptor_match(orc[a].descriptors(), orc[b].descriptors(), 10000, 0.86)
        exp = ref.remove_outliers(orc[a].keypoints(), orc[b].keypoints(), raw, 1000, 0.05, 3.0)
        assert len(raw) >= 8 and np.array_equal(got[p], exp), p


def test_edge_cases(ctx, amd, six):
    k0, d0 = six[0]
    empty = (np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, 61), np.uint8))
    few = (k0[:5], d0[:5])                      # at most 5 matches: returned unchanged, nothing drawn
    kc = k0.copy()
    kc["y"] = 2.0 * kc["x"]                     # collinear: most samples rank-deficient
    feats = [six[0], six[1], empty, few, (kc, d0), six[2]]
    pairs = [(0, 1), (2, 1), (1, 2), (3, 1), (0, 1), (2, 2), (4, 1), (1, 3), (5, 0), (3, 3), (4, 5)]
    for trials, eps in ((1000, 3.0), (2000, 3.0), (0, 0.5), (8, 10.0)):
        got = _same_as_loop(ctx, amd, feats, pairs, 0.86, trials, eps, seed=(1, 2))
        assert len(got[1]) == len(got[2]) == len(got[5]) == 0
    # 1-, 2- and 3-channel extractions: 21 / 41 / 61-byte descriptors
    for ch in (1, 2, 3):
        feats = [_feat(ctx, amd, 960, 540, 4, shift=(5 * i, 2 * i), descriptor_channels=ch) for i in range(3)]
        assert feats[0][1].shape[1] == {1: 21, 2: 41, 3: 61}[ch]
        _same_as_loop(ctx, amd, feats, [(0, 1), (1, 2), (2, 0), (1, 0)], 0.86, 1000, 3.0)


def test_64_byte_rows_compare_every_byte(ctx, amd):
    """desc_bytes 64: bytes 61..63 decide the matches (the pair matcher of akz_descriptor_match, not the 61-byte scan)."""
    rng = np.random.default_rng(5)
    n = 600
    base = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    base[:, 61:] = 0
    other = base.copy()
    other[:, :61] = base[rng.permutation(n)][:, :61]  # same first 61 bytes, shuffled
    other[:, 61:] = base[:, :3] ^ 0x5A
    d0 = base.copy()
    d0[:, 61:] = base[:, :3] ^ 0x5A
    d1 = np.concatenate([other, base])
    k0 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k0["x"] = rng.uniform(0, 800, n)
    k0["y"] = rng.uniform(0, 600, n)
    k1 = np.zeros(2 * n, amd.KEYPOINT_DTYPE)
    k1["x"] = np.concatenate([k0["x"] + 3.0, k0["x"]])
    k1["y"] = np.concatenate([k0["y"] + 1.0, k0["y"]])
    feats = [(k0, d0), (k1, d1)]
    got = _same_as_loop(ctx, amd, feats, [(0, 1), (1, 0), (0, 0)], 0.95, 500, 5.0)
    short = ctx.descriptor_match(d0[:, :61], d1[:, :61], 10000, 0.95)
    full = ctx.descriptor_match(d0, d1, 10000, 0.95)
    assert not np.array_equal(short, full) and len(got[0]) > 0


def test_scale_256_pairs(ctx, amd):
    feats = [_feat(ctx, amd, 640, 360, 3, shift=(3 * i, i)) for i in range(17)]
    pairs = list(itertools.permutations(range(17), 2))
    assert len(pairs) >= 256
    drawing = sum(len(ctx.descriptor_match(feats[a][1], feats[b][1], 10000, 0.86)) >= 8 for a, b in pairs)
    assert drawing * 1000 >= 250000
    _same_as_loop(ctx, amd, feats, pairs, 0.86, 1000, 3.0)


def test_second_context_beside_extraction(ctx, amd, six):
    import torch
    other = amd.Context(0, torch.cuda.Stream().cuda_stream)
    try:
        pairs = [(0, 1), (1, 2), (2, 3), (3, 0)]
        amd.random_seed(3, 4)
        exp = _loop(ctx, amd, six, pairs, 0.86, 1000, 3.0)
        frames = torch.from_numpy(np.stack([amd.synth_frame(1920, 1080, 40 + i) for i in range(4)])).cuda()
        job = ctx.extract_begin(frames, keep_all_planes=False)
        amd.random_seed(3, 4)
        got = other.match_features_pairs(six, pairs, 0.86, 1000, 3.0)
        res = job.finish()
        assert res.counts(0)[1] > 0
        for g, e in zip(got, exp):
            assert np.array_equal(g, e)
    finally:
        other.close()
