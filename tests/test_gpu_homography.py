"""The homography RANSAC on the GPU (akz_match_features_homography / _pairs): the device result equals the host path
(akz_remove_outliers_homography, the same model source) bit for bit -- kept list, H, found and the random source's state --,
the pairs call equals the loop of single-pair calls, the edges hold, the synthetic correspondences come out exact, and a real
projective warp is recovered."""
import numpy as np
import pytest

from test_gpu_match_pairs import _color, _feat, _pair_list
from test_homography_host import synthetic_case

pytestmark = pytest.mark.gpu


def _hbits(h):
    return None if h is None else np.asarray(h, np.float32).view(np.uint32).copy()


def _same(got, exp, what):
    (gm, gh), (em, eh) = got, exp
    assert gm.dtype == em.dtype and np.array_equal(gm, em), (what, len(gm), len(em))
    assert (gh is None) == (eh is None), what
    if gh is not None:
        assert np.array_equal(_hbits(gh), _hbits(eh)), (what, gh, eh)


@pytest.fixture(scope="module")
def six(ctx, amd):
    sizes = [(960, 540), (1280, 720)]
    return [_feat(ctx, amd, *sizes[i % 2], 21, shift=(7 * i, 3 * i)) for i in range(6)]


def _host(ctx, amd, fa, fb, ratio, trials, eps):
    raw = ctx.descriptor_match(fa[1], fb[1], 10000, ratio)
    return amd.remove_outliers_homography(fa[0], fb[0], raw, trials, amd.HOMOGRAPHY_EPSILON_MODEL, eps)


@pytest.mark.parametrize("trials", [0, 1, 8, 997, 1000, 4000])
def test_device_equals_host(ctx, amd, six, trials):
    found_any = False
    for eps in (0.0, 0.5, 3.0, 10.0):
        for ratio in (0.6, 0.86):
            for a, b in ((0, 2), (1, 3), (3, 5), (0, 1)):
                amd.random_seed(42, 69)
                got = amd.match_features_homography(six[a][0], six[a][1], six[b][0], six[b][1], ratio, trials, eps, ctx=ctx)
                after_dev = _color(amd)
                amd.random_seed(42, 69)
                exp = _host(ctx, amd, six[a], six[b], ratio, trials, eps)
                after_host = _color(amd)
                _same(got, exp, (a, b, trials, eps, ratio))
                assert after_dev == after_host, (a, b, trials, eps, ratio)
                found_any |= got[1] is not None
    assert found_any == (trials > 0)


def _loop(ctx, amd, feats, pairs, ratio, trials, eps):
    return [amd.match_features_homography(feats[a][0], feats[a][1], feats[b][0], feats[b][1], ratio, trials, eps, ctx=ctx)
            for a, b in pairs]


def _pairs_equal_loop(ctx, amd, feats, pairs, ratio, trials, eps, seed=(42, 69)):
    amd.random_seed(*seed)
    got = ctx.match_features_homography_pairs(feats, pairs, ratio, trials, eps)
    after_batch = _color(amd)
    amd.random_seed(*seed)
    exp = _loop(ctx, amd, feats, pairs, ratio, trials, eps)
    after_loop = _color(amd)
    assert len(got) == len(exp) == len(pairs)
    for p, (g, e) in enumerate(zip(got, exp)):
        _same(g, e, (p, pairs[p], trials, eps, ratio))
    assert after_batch == after_loop, (trials, eps, ratio)
    return got


@pytest.mark.parametrize("trials,eps,ratio", [(1000, 3.0, 0.86), (0, 0.5, 0.6), (8, 10.0, 0.86), (4000, 3.0, 0.6),
                                              (997, 0.0, 0.86)])
def test_pairs_equal_loop(ctx, amd, six, trials, eps, ratio):
    got = _pairs_equal_loop(ctx, amd, six, _pair_list(), ratio, trials, eps)
    if trials and eps > 0:
        assert any(h is not None for _, h in got)
    # the module-level twin
    amd.random_seed(42, 69)
    twin = amd.match_features_homography_pairs(six, _pair_list()[:5], ratio, trials, eps, ctx=ctx)
    for g, e in zip(twin, got[:5]):
        _same(g, e, "twin")


def test_pairs_edge_cases(ctx, amd, six):
    k0, d0 = six[0]
    empty = (np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, 61), np.uint8))
    few = (k0[:3], d0[:3])                      # at most 3 matches: returned unchanged, nothing drawn
    kc = k0.copy()
    kc["y"] = 2.0 * kc["x"]                     # every keypoint on one line: every sample degenerate
    feats = [six[0], six[1], empty, few, (kc, d0), six[2]]
    pairs = [(0, 1), (2, 1), (1, 2), (3, 1), (0, 1), (2, 2), (4, 1), (1, 4), (1, 3), (5, 0), (3, 3), (4, 5)]
    for trials, eps in ((1000, 3.0), (2000, 3.0), (0, 0.5), (8, 10.0)):
        got = _pairs_equal_loop(ctx, amd, feats, pairs, 0.86, trials, eps, seed=(1, 2))
        assert len(got[1][0]) == len(got[2][0]) == len(got[5][0]) == 0
        for p in (6, 7):                        # the line: all kept, no model
            a, b = pairs[p]
            raw = ctx.descriptor_match(feats[a][1], feats[b][1], 10000, 0.86)
            assert len(raw) >= 4 and np.array_equal(got[p][0], raw) and got[p][1] is None, p
        raw = ctx.descriptor_match(few[1], six[1][1], 10000, 0.86)
        assert len(raw) < 4 and np.array_equal(got[3][0], raw) and got[3][1] is None
    # 1-, 2- and 3-channel extractions: 21 / 41 / 61-byte descriptors
    for ch in (1, 2, 3):
        feats = [_feat(ctx, amd, 960, 540, 4, shift=(5 * i, 2 * i), descriptor_channels=ch) for i in range(3)]
        assert feats[0][1].shape[1] == {1: 21, 2: 41, 3: 61}[ch]
        _pairs_equal_loop(ctx, amd, feats, [(0, 1), (1, 2), (2, 0), (1, 0)], 0.86, 1000, 3.0)


def test_pairs_64_byte_rows(ctx, amd):
    rng = np.random.default_rng(5)
    n = 600
    base = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    d1 = np.concatenate([base[rng.permutation(n)], base])
    d1[:n, 61:] ^= 0x5A                         # the first copies differ only in bytes 61..63
    k0 = np.zeros(n, amd.KEYPOINT_DTYPE)
    k0["x"] = rng.uniform(0, 800, n)
    k0["y"] = rng.uniform(0, 600, n)
    k1 = np.zeros(2 * n, amd.KEYPOINT_DTYPE)
    k1["x"] = np.concatenate([rng.uniform(0, 800, n), k0["x"] + 3.0])
    k1["y"] = np.concatenate([rng.uniform(0, 600, n), k0["y"] + 1.0])
    got = _pairs_equal_loop(ctx, amd, [(k0, base), (k1, d1)], [(0, 1), (1, 0), (0, 0)], 0.95, 500, 5.0)
    assert len(got[0][0]) > 0 and got[0][1] is not None


def _descriptor_case(amd, seed):
    """synthetic_case with descriptors that make descriptor_match return exactly its matches (index_0 ascending)."""
    k0, k1, m, inl, h = synthetic_case(amd, seed)
    order = np.argsort(m["index_0"])
    m, inl = m[order], inl[order]
    rng = np.random.default_rng(1000 + seed)
    dsc = rng.integers(0, 256, (len(m), 61), dtype=np.uint8)
    d0 = np.zeros_like(dsc)
    d1 = np.zeros_like(dsc)
    d0[m["index_0"]] = dsc
    d1[m["index_1"]] = dsc
    m["distance"] = 0.0
    return k0, d0, k1, d1, m, inl


@pytest.mark.parametrize("seed", range(6))
def test_synthetic_correspondences_exact(ctx, amd, seed):
    k0, d0, k1, d1, m, inl = _descriptor_case(amd, seed)
    raw = ctx.descriptor_match(d0, d1, 10000, 0.86)
    assert np.array_equal(raw["index_0"], m["index_0"]) and np.array_equal(raw["index_1"], m["index_1"])
    amd.random_seed(42, 69)
    kept, h = amd.match_features_homography(k0, d0, k1, d1, 0.86, 1000, 2.0, ctx=ctx)
    assert h is not None
    assert np.array_equal(kept, raw[inl]), (len(kept), int(inl.sum()))
    amd.random_seed(42, 69)
    (kp, hp), = ctx.match_features_homography_pairs([(k0, d0), (k1, d1)], [(0, 1)], 0.86, 1000, 2.0)
    assert np.array_equal(kp, kept) and np.array_equal(_hbits(hp), _hbits(h))


# ---- a real projective warp ----------------------------------------------------------------------------------------------
WARP_W, WARP_H, WARP_IDX = 1280, 720, 5


def warp_case(amd, idx=WARP_IDX):
    """synth_frame(1280, 720, idx) and its nearest-neighbour warp by H_true (8 degrees, scale 0.9, perspective 1e-4, about the
    frame's centre): image 1 at p holds image 0 at H_true^-1 p (0 outside).  Returns (frame 0, frame 1, H_true with
    H[2, 2] = 1)."""
    f0 = amd.synth_frame(WARP_W, WARP_H, idx)
    c = np.array([[1, 0, WARP_W / 2], [0, 1, WARP_H / 2], [0, 0, 1.0]])
    ci = np.array([[1, 0, -WARP_W / 2], [0, 1, -WARP_H / 2], [0, 0, 1.0]])
    a = np.deg2rad(8.0)
    r = np.array([[0.9 * np.cos(a), -0.9 * np.sin(a), 0], [0.9 * np.sin(a), 0.9 * np.cos(a), 0], [0, 0, 1.0]])
    p = np.array([[1, 0, 0], [0, 1, 0], [1e-4, 0, 1.0]])
    h = c @ r @ p @ ci
    h = h / h[2, 2]
    ys, xs = np.mgrid[0:WARP_H, 0:WARP_W]
    q = np.linalg.inv(h) @ np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)])
    sx, sy = np.rint(q[0] / q[2]).astype(np.int64), np.rint(q[1] / q[2]).astype(np.int64)
    ok = (q[2] > 0) & (sx >= 0) & (sx < WARP_W) & (sy >= 0) & (sy < WARP_H)
    f1 = np.zeros(WARP_H * WARP_W, np.uint8)
    f1[ok] = f0[sy[ok], sx[ok]]
    return f0, f1.reshape(WARP_H, WARP_W), h


def inlier_rule(h, k0, k1, matches, eps):
    """The error rule of include/akaze_hip.h in numpy float32, in its expression order."""
    h = np.asarray(h, np.float32).reshape(9)
    x0 = k0["x"][matches["index_0"]].astype(np.float32)
    y0 = k0["y"][matches["index_0"]].astype(np.float32)
    x1 = k1["x"][matches["index_1"]].astype(np.float32)
    y1 = k1["y"][matches["index_1"]].astype(np.float32)
    w = (h[6] * x0 + h[7] * y0) + h[8]
    u = (h[0] * x0 + h[1] * y0) + h[2]
    v = (h[3] * x0 + h[4] * y0) + h[5]
    du, dv, ew = u - x1 * w, v - y1 * w, np.float32(eps) * w
    return (w > 0) & (du * du + dv * dv < ew * ew)


def h_true_consistent(k0, k1, matches, h, eps):
    return inlier_rule(np.asarray(h, np.float32), k0, k1, matches, eps)


def test_real_warp(ctx, amd):
    """Frame 5 and its warp.  On the oracle's features (extract + descriptor_match at ratio 0.86 on the CPU) 287 of the 337
    raw matches (85 %) are consistent with H_true at 3 px.  Here: a model is found, every kept match passes the error rule under the
    returned H, and the kept list holds at least 90 % of the raw matches that H_true accepts."""
    import torch
    f0, f1, h_true = warp_case(amd)
    res = [ctx.extract_features(f, keep_all_planes=False) for f in (f0, f1)]
    (k0, d0), (k1, d1) = [(r.keypoints(), r.descriptors()) for r in res]
    raw = ctx.descriptor_match(d0, d1, 10000, 0.86)
    amd.random_seed(42, 69)
    kept, h = amd.match_features_homography(k0, d0, k1, d1, 0.86, 1000, 3.0, ctx=ctx)
    assert h is not None
    assert np.all(inlier_rule(h, k0, k1, kept, 3.0))
    truth = raw[h_true_consistent(k0, k1, raw, h_true, 3.0)]
    both = np.isin(truth["index_0"], kept["index_0"]).sum()
    print("raw", len(raw), "H_true-consistent", len(truth), "kept", len(kept), "of those kept", both)
    assert len(truth) > 0 and both >= 0.9 * len(truth)
    torch.cuda.synchronize()
