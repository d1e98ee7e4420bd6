"""Cross-checked matching on the GPU (akz_descriptor_match_cross, akz_descriptor_match_cross_device,
akz_match_features_seeded_cross_pairs): the lists equal the host statement akz_descriptor_match_cross_host and the oracle's
descriptor_match called twice and intersected in Python, bit for bit -- on the planted sets of tests/test_cross_match_host.py,
at the edges of k_pairs_cross_filter's rounds of 256 records (forward lists of 0, 1, 255, 256, 257 and about 1 000), of its
binary search (reverse lists of 0 .. 5 records and of a length that is no power of two, with hits on their first and last
record), of the matcher's tiles (set sizes around launch::match_mfma_tile_rows(), read from the library), for rows
of 61 and 64 bytes and the matcher modes 0, 1 and 2.  The composite equals akz_remove_outliers_seeded over the host statement's
list with the pair's stream, the batch equals the loop of one-pair calls, the thread's random source is untouched,
cross_check=False is the call as it was, and refusals come before any GPU work."""
import ctypes as C

import numpy as np
import pytest

from test_cross_match_host import KINDS, _flip, check_kinds, cross_scene, oracle_cross, planted_sets
from test_gpu_match_pairs import _color
from test_gpu_seeded_ransac import RATIO, _pair_sets, grid_epsilon, seed_of
from test_seeded_ransac_host import K, options, planted, same4

pytestmark = pytest.mark.gpu


def tile_rows(amd):
    """launch::match_mfma_tile_rows(), from the library (akz_debug_match_tile_rows): a retuned tile moves the sizes with it"""
    rows = C.c_uint32()
    assert amd.lib().akz_debug_match_tile_rows(C.byref(rows)) == 0 and rows.value >= 2
    return rows.value


def rows64(d):
    r = np.zeros((len(d), 64), np.uint8)
    r[:, :d.shape[1]] = d
    return r


def device_list(ctx, amd, a, b, thr, ratio):
    """descriptor_match_cross_device on 64-byte rows.  The device form is that of akz_descriptor_match_device: it takes M-LDB rows,
    whose bytes 61..63 are padding that is NOT compared -- so it is held to the statement for rows of at most 61 bytes only; rows of
    62..64 bytes go through the host-array form, which compares every byte (hold, below)."""
    import torch
    da = torch.from_numpy(rows64(a) if len(a) else np.zeros((0, 64), np.uint8)).cuda()
    db = torch.from_numpy(rows64(b) if len(b) else np.zeros((0, 64), np.uint8)).cuda()
    out, cnt = ctx.descriptor_match_cross_device(da, db, thr, ratio)
    ctx.synchronize()
    n = int(cnt.item())
    assert 0 <= n <= len(a)
    return out.cpu().numpy()[:n].copy().view(amd.MATCH_DTYPE).reshape(-1)


def hold(ctx, amd, ref, a, b, thr, ratio, what):
    """every GPU form against the host statement and the oracle intersection -> (cross, fwd, rev)"""
    exp, fwd, rev = oracle_cross(ref, a, b, thr, ratio)
    host = amd.descriptor_match_cross_host(a, b, thr, ratio)
    assert np.array_equal(host, exp), (what, "host", len(host), len(exp))
    got = ctx.descriptor_match_cross(a, b, thr, ratio)
    assert got.dtype == exp.dtype and np.array_equal(got, exp), (what, "host arrays", len(got), len(exp))
    if a.shape[1] <= 61:
        dev = device_list(ctx, amd, a, b, thr, ratio)
        assert np.array_equal(dev, exp), (what, "device rows", len(dev), len(exp))
    return exp, fwd, rev


# forward lists of 0, 1, 255, 256, 257 and about 1 000 records at ratio 0.86: (mutual, rival, reverse_ratio, tie) -- the forward
# list holds mutual + 2 (rival + reverse_ratio + tie) records, the reverse list mutual + rival
FORWARD = {0: (0, 0, 0, 0), 1: (1, 0, 0, 0), 255: (243, 2, 2, 2), 256: (244, 2, 2, 2), 257: (245, 2, 2, 2), 1001: (941, 10, 10, 10)}
# reverse lists of 0 .. 5 records and of 11
REVERSE = {0: (0, 0, 2, 2), 1: (1, 0, 1, 1), 2: (1, 1, 1, 1), 3: (2, 1, 1, 1), 4: (2, 2, 1, 1), 5: (3, 2, 1, 1), 11: (8, 3, 2, 2)}


@pytest.mark.parametrize("mode", [2, 1, 0])
@pytest.mark.parametrize("nb", [61, 64])
def test_full_sets(ctx, amd, ref, mode, nb):
    a, b, kind_a, base_a, kind_b = planted_sets(1600 + nb, nb)
    ctx.set_match_mode(mode)
    try:
        for ratio in (0.86, 1.0, 2.0):
            cross, fwd, _ = hold(ctx, amd, ref, a, b, 10000, ratio, (mode, nb, ratio))
            check_kinds(cross, fwd, kind_a, base_a, kind_b, ratio)
            cut, fwd_cut, _ = hold(ctx, amd, ref, a, b, 8, ratio, (mode, nb, ratio, "threshold 8"))
            assert 0 < len(cut) and len(fwd_cut) < len(fwd)
        cross, fwd, _ = hold(ctx, amd, ref, a, a, 10000, RATIO, (mode, nb, "cross(A, A)"))
        assert len(cross) == len(fwd) == len(a)
        for x, y in ((a[:0], b), (a, b[:0]), (a[:0], b[:0])):
            assert len(hold(ctx, amd, ref, x, y, 10000, RATIO, (mode, nb, "empty"))[0]) == 0
    finally:
        ctx.set_match_mode(2)


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_filter_rounds_and_search_edges(ctx, amd, ref, mode):
    ctx.set_match_mode(mode)
    try:
        for nb in (61, 64):
            # (a forward list of 0 or 1 records and a reverse list of 0 or 1 cannot hold every kind: those cases are the edges
            # alone; every other case holds all six kinds and drops some but not all of its forward list)
            for n_fwd, (mu, ri, rr, ti) in FORWARD.items():
                a, b, kind_a, _, kind_b = planted_sets(3000 + n_fwd, nb, mutual=mu, rival=ri, reverse_ratio=rr, tie=ti, orphan=3, stranger=5)
                cross, fwd, rev = hold(ctx, amd, ref, a, b, 10000, RATIO, (mode, nb, "forward", n_fwd))
                assert len(fwd) == n_fwd and len(rev) == mu + ri and len(cross) == mu + ri
                if n_fwd > 1:
                    assert set(kind_a) | set(kind_b) == set(KINDS) and 0 < len(cross) < len(fwd)
            for n_rev, (mu, ri, rr, ti) in REVERSE.items():
                a, b, kind_a, _, kind_b = planted_sets(4000 + n_rev, nb, mutual=mu, rival=ri, reverse_ratio=rr, tie=ti, orphan=2, stranger=3)
                cross, fwd, rev = hold(ctx, amd, ref, a, b, 10000, RATIO, (mode, nb, "reverse", n_rev))
                assert len(rev) == n_rev and len(cross) == n_rev < len(fwd)
                if n_rev > 1:
                    assert set(kind_a) | set(kind_b) == set(KINDS) and 0 < len(cross)
                if n_rev:        # the search ends on the reverse list's first and on its last record
                    assert {int(rev[0]["index_0"]), int(rev[-1]["index_0"])} <= set(cross["index_1"].tolist())
    finally:
        ctx.set_match_mode(2)


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_set_sizes_around_the_tile(ctx, amd, ref, mode):
    """n0 and n1 each one below, at and one above the matcher's tile, n0 != n1 in both orders: prefixes of the two
    sets of one planted case with more than a tile of rows on either side.  Every case holds all six kinds and is held
    to `0 < len(cross) < len(fwd)`.  Rows of 61 bytes: the tiles are those of the matrix-core matcher, which rows of 62..64 bytes
    never reach (they take the pair matcher of akz_descriptor_match, whatever the sizes)."""
    tile = tile_rows(amd)
    a, b, kind_a, base_a, kind_b = planted_sets(5000, 61, mutual=tile, rival=8, reverse_ratio=8, tie=8, orphan=10, stranger=30)
    assert len(a) >= tile + 1 and len(b) >= tile + 1
    ctx.set_match_mode(mode)
    try:
        for n0 in (tile - 1, tile, tile + 1):
            for n1 in (tile - 1, tile, tile + 1):
                if n0 == n1:
                    continue
                present = set(kind_a[:n0]) | {k for j, k in enumerate(kind_b[:n1]) if k == "orphan" or not np.any(base_a[:n0] == j)}
                assert set(kind_a[:n0]) >= set(KINDS) - {"orphan"} and "orphan" in present, (n0, n1)
                for ratio in (RATIO, 2.0):
                    cross, fwd, _ = hold(ctx, amd, ref, a[:n0], b[:n1], 10000, ratio, (mode, n0, n1, ratio))
                    assert 0 < len(cross) < len(fwd), (mode, n0, n1, ratio)
    finally:
        ctx.set_match_mode(2)


# ---- the composite ----------------------------------------------------------------------------------------------------------
def _cross_pair_sets(amd, model, nb=61):
    """the sets and the pair list of the seeded test (_pair_sets: a repeated pair, both orders, (a, a), unrelated sets, a pair
    below K, an empty set on either side), with first sets that also hold rivals (cross_scene): sets 0 / 1, 2 / 3 of 257 and 65
    matches and 64 / 16 rivals; sets 4 / 5: K + 1 forward matches of which two are rivals -- K - 1 after the cross-check --; set 8:
    another second set for set 0, so that set 0's grouped launch carries reverse lists of 257, 300, 0 and 260 rows"""
    cases = {(model, n): planted(amd, model, n, seed_of(model, n)) for n in (257, 65, K[model] - 1)} if nb == 61 else None
    feats, pairs = _pair_sets(amd, cases, model, nb)
    for first, n in ((0, 257), (2, 65)):
        fa, fb = cross_scene(amd, model, n, seed_of(model, n), nb)
        assert np.array_equal(fb[1], feats[first + 1][1]) and np.array_equal(fa[1][:n], feats[first][1])
        feats[first] = fa
    small = K[model] - 1
    k4, d4 = feats[4]
    rng = np.random.default_rng(5)
    rd = np.array([_flip(feats[5][1][np.flatnonzero((feats[5][1] == d4[t]).all(1))[0]], rng.permutation(480)[:30]) for t in range(2)])
    rk = k4[:2].copy()
    rk["x"] += 40.0
    feats[4] = (np.concatenate([k4[:small], rk]), np.concatenate([d4[:small], rd]))
    rng = np.random.default_rng(8)            # set 8: set 1 in reverse order and three unrelated rows
    k8 = np.zeros(3, amd.KEYPOINT_DTYPE)
    k8["x"], k8["y"] = rng.uniform(0, 1920, 3), rng.uniform(0, 1080, 3)
    n1 = len(feats[1][1])
    feats.append((np.concatenate([feats[1][0][:n1][::-1], k8]), np.concatenate([feats[1][1][::-1], rng.integers(0, 256, (3, nb), dtype=np.uint8)])))
    return feats, pairs + [(0, 8), (8, 0)]


@pytest.mark.parametrize("model,nb,conf,its", [("H", 61, 0.99, 2), ("H", 61, 0.0, 0), ("F", 61, 0.99, 0), ("F", 61, 0.0, 2),
                                               ("F", 64, 0.99, 2), ("H", 64, 0.0, 0)])
def test_composite_equals_the_host_statement_and_the_loop(ctx, amd, ref, model, nb, conf, its):
    feats, pairs = _cross_pair_sets(amd, model, nb)
    opt = options(amd, model, max_trials=513, confidence=conf, refine_iterations=its, stream_base=(1 << 64) - 3, lowes_ratio=RATIO,
                  epsilon_inliers=grid_epsilon(model, conf))
    if model == "F":
        opt = opt.copy(model_kind=amd.RANSAC_FUNDAMENTAL_NORMALISED, epsilon_inliers=2.0)        # kind 3
    amd.random_seed(42, 69)
    fresh = _color(amd)
    amd.random_seed(42, 69)
    got = ctx.match_features_seeded_pairs(feats, pairs, opt, cross_check=True)
    assert _color(amd) == fresh                                   # the thread's source: neither read nor advanced
    plain = ctx.match_features_seeded_pairs(feats, pairs, opt)
    assert len(got) == len(pairs)
    shorter = 0
    for p, (a, b) in enumerate(pairs):
        one = opt.copy(stream_base=(opt.stream_base + p) & ((1 << 64) - 1))
        raw = amd.descriptor_match_cross_host(feats[a][1], feats[b][1], 10000, RATIO)
        exp, fwd, _ = oracle_cross(ref, feats[a][1], feats[b][1], 10000, RATIO)
        assert np.array_equal(raw, exp), p
        same4(got[p], amd.remove_outliers_seeded(feats[a][0], feats[b][0], raw, opt, stream=one.stream_base), ("host", p))
        same4(got[p], ctx.match_features_seeded_pairs([feats[a], feats[b]], [(0, 1)], one, cross_check=True)[0], ("loop", p))
        same4(plain[p], amd.remove_outliers_seeded(feats[a][0], feats[b][0], fwd, opt, stream=one.stream_base), ("plain", p))
        shorter += len(raw) < len(fwd)
    assert shorter >= 6                                           # (0, 1) five times and (2, 3): their rivals are gone
    assert all(got[p][1] is not None for p in (0, 1, 2, 3, 9, 10, 11, 12))
    # below K only after the cross-check: the plain call runs its trials on K + 1 matches, this one returns the K - 1 unchanged
    assert got[6][1] is None and got[6][3] == 0 and len(got[6][0]) == K[model] - 1 and plain[6][3] > 0
    assert all(got[p][3] == 0 and len(got[p][0]) == 0 for p in (7, 8))
    one = amd.match_features_seeded(*feats[0], *feats[1], opt, ctx=ctx, cross_check=True)
    same4(one, ctx.match_features_seeded_pairs(feats, pairs[:1], opt.copy(), cross_check=True)[0], "one pair")
    twin = amd.match_features_seeded_pairs(feats, pairs[:3], opt, ctx=ctx, cross_check=True)
    for g, e in zip(twin, got[:3]):
        same4(g, e, "twin")


@pytest.mark.parametrize("model", ["H", "F"])
def test_guided_stage_stays_one_directional(ctx, amd, model):
    feats, pairs = _cross_pair_sets(amd, model)
    plain = options(amd, model, max_trials=300, refine_iterations=2, stream_base=11, lowes_ratio=RATIO, epsilon_inliers=grid_epsilon(model, 0.99))
    ref_ = ctx.match_features_seeded_pairs(feats, pairs, plain, cross_check=True)
    got = ctx.match_features_seeded_pairs(feats, pairs, plain.copy(guided=1, guided_radius=3.0, guided_lowes_ratio=RATIO), cross_check=True)
    from test_seeded_ransac_host import KIND
    n_guided = 0
    for p, ((a, b), g, r) in enumerate(zip(pairs, got, ref_)):
        fa, fb = feats[a], feats[b]
        em = r[0] if r[1] is None else amd.descriptor_match_guided_host(fa[0], fa[1], fb[0], fb[1], r[1], KIND[model], 3.0, 10000, RATIO)
        same4(g, (em, *r[1:]), p)
        n_guided += r[1] is not None
    assert n_guided >= 6


def test_cross_check_off_is_the_call_as_it_was(ctx, amd):
    for model in ("H", "F"):
        feats, pairs = _cross_pair_sets(amd, model)
        opt = options(amd, model, max_trials=300, refine_iterations=2, stream_base=7, lowes_ratio=RATIO, epsilon_inliers=grid_epsilon(model, 0.99))
        a = ctx.match_features_seeded_pairs(feats, pairs, opt)
        ctx.match_features_seeded_pairs(feats, pairs, opt, cross_check=True)      # (its scratch and tables in between change nothing)
        b = ctx.match_features_seeded_pairs(feats, pairs, opt, cross_check=False)
        for p, (x, y) in enumerate(zip(a, b)):
            same4(x, y, p)
            fa, fb = feats[pairs[p][0]], feats[pairs[p][1]]
            raw = ctx.descriptor_match(fa[1], fb[1], 10000, RATIO)
            same4(x, amd.remove_outliers_seeded(fa[0], fb[0], raw, opt, stream=7 + p), ("host", p))


def test_refusals_come_before_any_gpu_work(ctx, amd):
    feats, pairs = _cross_pair_sets(amd, "F")
    good = options(amd, "F", max_trials=128)
    more = list(feats)
    more[3] = (feats[3][0][:10], feats[3][1])              # more descriptors than keypoints, in the second pair
    calls = [(feats, pairs, None), (feats, pairs, good.copy(struct_size=72)), (feats, pairs, good.copy(model_kind=7)),
             (feats, pairs, good.copy(max_trials=(1 << 24) + 1)), (feats, pairs, good.copy(confidence=1.0)),
             (feats, pairs, good.copy(confidence=float("nan"))), (feats, pairs, good.copy(guided=1, guided_radius=-1.0)),
             (feats, pairs + [(0, 10)], good), (more, pairs, good)]
    amd.random_seed(42, 69)
    fresh = _color(amd)
    L = amd.lib()
    for k, (fs, pr, opt) in enumerate(calls):
        a = amd._PairsArgs(ctx, fs, pr)
        a.out["index_0"], a.n[:] = 77, 12345
        f = np.full((len(a.pr), 9), 7.0, np.float32)
        found, it, run = (np.full(len(a.pr), 55, t) for t in (np.int32, np.uint32, np.uint64))
        amd.random_seed(42, 69)
        status = L.akz_match_features_seeded_cross_pairs(*a.head, C.byref(opt) if opt is not None else None, *a.tail,
                                                         f.ctypes.data_as(C.POINTER(C.c_float)), found.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         it.ctypes.data_as(C.POINTER(C.c_uint32)), run.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert status != 0, k
        assert np.all(a.out["index_0"] == 77) and np.all(a.n == 12345) and np.all(f == 7.0), k    # nothing was written
        assert np.all(found == 55) and np.all(it == 55) and np.all(run == 55), k
        assert _color(amd) == fresh, k
    # the pair calls: the refusals of akz_descriptor_match, nothing written
    a, b = planted_sets(1661, 61)[:2]
    out = np.zeros(len(a), amd.MATCH_DTYPE)
    out["index_0"] = 77
    n = C.c_uint64(12345)
    pa, pb, po = a.ctypes.data, b.ctypes.data, out.ctypes.data
    for k, args in enumerate(((None, len(a), pb, len(b), 61, 10000, 0.86, po, C.byref(n)), (pa, len(a), None, len(b), 61, 10000, 0.86, po, C.byref(n)),
                              (pa, len(a), pb, len(b), 61, 10000, 0.86, None, C.byref(n)), (pa, len(a), pb, len(b), 61, 10000, 0.86, po, None),
                              (pa, len(a), pb, len(b), 0, 10000, 0.86, po, C.byref(n)), (pa, len(a), pb, len(b), 65, 10000, 0.86, po, C.byref(n)))):
        assert L.akz_descriptor_match_cross(ctx._h, *args) != 0, k
        assert n.value == 12345 and np.all(out["index_0"] == 77), k
    import torch
    da, db = torch.from_numpy(rows64(a)).cuda(), torch.from_numpy(rows64(b)).cuda()
    d_out = torch.full((len(a), 24), 9, dtype=torch.uint8).cuda()
    d_n = torch.full((1,), 12345, dtype=torch.int64).cuda()
    for k, args in enumerate(((None, len(a), db.data_ptr(), len(b), 10000, 0.86, d_out.data_ptr(), d_n.data_ptr()),
                              (da.data_ptr(), len(a), None, len(b), 10000, 0.86, d_out.data_ptr(), d_n.data_ptr()),
                              (da.data_ptr(), len(a), db.data_ptr(), len(b), 10000, 0.86, None, d_n.data_ptr()),
                              (da.data_ptr(), len(a), db.data_ptr(), len(b), 10000, 0.86, d_out.data_ptr(), None),
                              (da.data_ptr(), 1 << 31, db.data_ptr(), len(b), 10000, 0.86, d_out.data_ptr(), d_n.data_ptr()))):
        assert L.akz_descriptor_match_cross_device(ctx._h, *args) != 0, k
    ctx.synchronize()
    assert int(d_n.item()) == 12345 and bool((d_out == 9).all())
