"""akz_match_features_seeded_pose_pairs on the GPU: every pair equals the host composite -- akz_remove_outliers_seeded on the
pair's raw list (descriptor_match, or cross(A, B) with cross_check), then, where a model was found, akz_recover_pose_host with
that list, that model and the two sets' cameras -- bit for bit: the list, the model, found, iterations, trials_run, every word of
the pose and of the points.  The feature sets are the planted two-view scenes of tests/test_seeded_ransac_host.py, so the raw
lists are known; every set has a camera of its own (a shared one would hide a K0 / K1 mix-up)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_fundamental_refit import SEEDS as SEEDS_F
from test_seeded_ransac_host import planted

pytestmark = pytest.mark.gpu

RATIO = 0.86
SIZES = (7, 8, 9, 255, 256, 257, 1000)   # below K, K, the 256-lane boundaries, several strides (0: pair 7 below)
BASE = 5                                 # stream_base
# (model_kind, epsilon_inliers): the reference's trial model at the epsilon where its winners keep about half of a scene (some of
# them behind a camera: lists that shrink), the normalised one at 2 px (nearly all in front: lists that do not)
KINDS = {1: 4.0, 3: 2.0}


def camera(s):
    """the scenes' camera (f = 1200 px, centre 960, 540), a little different for every set"""
    return (1200.0 + 3 * s, 1200.0 - 2 * s, 960.0 + 1.5 * s, 540.0 - s)


@pytest.fixture(scope="module")
def world(amd):
    """sets 2 i, 2 i + 1: the planted case of SIZES[i] matches; set 14: empty; set 15: 300 rows unrelated to all.  Pairs 0 .. 6: the
    planted cases in order of size; 7: no match at all; 8: pair 5 again; 9: pair 5 reversed; 10: (a, a); 11: unrelated sets.
    (built once, left unchanged)"""
    feats = [f for n in SIZES for f in planted(amd, "F", n, SEEDS_F[n])[:2]]
    feats.append((np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, 61), np.uint8)))
    rng = np.random.default_rng(99)
    k = np.zeros(300, amd.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 1920, 300), rng.uniform(0, 1080, 300)
    feats.append((k, rng.integers(0, 256, (300, 61), dtype=np.uint8)))
    pairs = [(2 * i, 2 * i + 1) for i in range(len(SIZES))] + [(10, 14), (10, 11), (11, 10), (8, 8), (12, 15)]
    return feats, [camera(s) for s in range(len(feats))], pairs


@pytest.fixture(scope="module")
def raw_lists(ctx, amd, world):
    """every pair's raw list, plain and cross-checked (computed once)"""
    feats, cams, pairs = world
    plain = [ctx.descriptor_match(feats[a][1], feats[b][1], 10000, RATIO) for a, b in pairs]
    cross = [amd.descriptor_match_cross_host(feats[a][1], feats[b][1], 10000, RATIO) for a, b in pairs]
    for i, n in enumerate(SIZES):
        assert len(plain[i]) == n and len(cross[i]) == n, (n, len(plain[i]), len(cross[i]))
    assert len(plain[7]) == 0 and len(plain[10]) == 256
    return {0: plain, 1: cross}


def options(amd, kind, its, **kw):
    return amd.RansacOptions(model_kind=kind, max_trials=200, confidence=0.0, refine_iterations=its, epsilon_inliers=KINDS[kind],
                             stream_base=BASE, lowes_ratio=RATIO, **kw)


def host_composite(amd, fa, fb, cam_a, cam_b, raw, opt, stream):
    """-> (list, model or None, fits, trials, pose words, points or None)"""
    kept, f, it, tr = amd.remove_outliers_seeded(fa[0], fb[0], raw, opt, stream=stream)
    if f is None:
        return kept, f, it, tr, np.zeros(21, np.uint32), None
    kept2, pose, pts = amd.recover_pose_host(fa[0], fb[0], kept, f, cam_a, cam_b, points=True)
    return kept2, f, it, tr, pose.words(), pts


def same(got, exp, what):
    gm, gf, gi, gt, gp, gx = got
    em, ef, ei, et, ep, ex = exp
    assert gm.dtype == em.dtype and np.array_equal(gm, em), (what, len(gm), len(em))
    assert (gf is None) == (ef is None), what
    if gf is not None:
        assert np.array_equal(np.asarray(gf, np.float32).view(np.uint32), np.asarray(ef, np.float32).view(np.uint32)), (what, gf, ef)
    assert (gi, gt) == (ei, et), (what, gi, ei, gt, et)
    assert np.array_equal(gp.words() if hasattr(gp, "words") else gp, ep), (what, gp.words() if hasattr(gp, "words") else gp, ep)
    assert (gx is None) == (ex is None), what
    if gx is not None:
        assert gx.shape == ex.shape and np.array_equal(gx.view(np.uint32), ex.view(np.uint32)), (what, np.abs(gx - ex).max())


@pytest.mark.parametrize("kind,its,cross", [(k, i, c) for k in (1, 3) for i in (0, 2) for c in (0, 1)])
def test_device_equals_host_statement_in_one_call(ctx, amd, world, raw_lists, kind, its, cross):
    feats, cams, pairs = world
    opt = options(amd, kind, its)
    got = ctx.match_features_seeded_pose_pairs(feats, cams, pairs, opt, cross_check=bool(cross), points=True)
    assert len(got) == len(pairs)
    posed = 0
    for p, (a, b) in enumerate(pairs):
        exp = host_composite(amd, feats[a], feats[b], cams[a], cams[b], raw_lists[cross][p], opt, BASE + p)
        same(got[p], exp, (kind, its, cross, p))
        pose = got[p][4]
        if got[p][1] is None:
            assert not pose.words().any(), p
        posed += pose.found
        if pose.found:
            assert len(got[p][0]) == pose.counts[pose.winner] == pose.counts.max() > 0, p
    assert got[0][1] is None and len(got[0][0]) == 7 and got[0][3] == 0          # below K: unchanged, nothing run, no pose
    assert len(got[7][0]) == 0 and got[7][1] is None                               # no match at all
    assert got[10][1] is None and not got[10][4].words().any()                     # (a, a): no trial has a model
    assert posed >= 6, posed
    assert got[8][4].found and got[9][4].found                                     # the repeated and the reversed pair have poses


def test_batch_equals_the_loop_of_one_pair_calls(ctx, amd, world):
    feats, cams, pairs = world
    opt = options(amd, 3, 2)
    got = ctx.match_features_seeded_pose_pairs(feats, cams, pairs, opt, points=True)
    for p, (a, b) in enumerate(pairs):
        one = ctx.match_features_seeded_pose_pairs([feats[a], feats[b]], [cams[a], cams[b]], [(0, 1)], opt.copy(stream_base=BASE + p), points=True)[0]
        same(got[p], (*one[:4], one[4].words(), one[5]), ("loop", p))
    # without the points: the same lists and poses; the module-level forms are the same call
    bare = amd.match_features_seeded_pose_pairs(feats, cams, pairs, opt, ctx=ctx)
    for p, (g, e) in enumerate(zip(bare, got)):
        assert len(g) == 5
        same((*g, e[5]), (*e[:4], e[4].words(), e[5]), ("bare", p))
    a, b = pairs[5]
    one = amd.match_features_seeded_pose(feats[a][0], feats[a][1], cams[a], feats[b][0], feats[b][1], cams[b], opt.copy(stream_base=BASE + 5), ctx=ctx)
    same((*one, got[5][5]), (*got[5][:4], got[5][4].words(), got[5][5]), "one pair")


def raw_call(ctx, amd, feats, cams, pairs, opt, cameras=True, poses=True, cross=0):
    """the ABI with every output prefilled -> (status, the arrays)"""
    a = amd._PairsArgs(ctx, feats, pairs)
    a.out["index_0"], a.out["index_1"], a.out["distance"] = 77, 78, 79.0
    a.n[:] = 12345
    f = np.full((len(a.pr), 9), 7.0, np.float32)
    found, it, run = (np.full(len(a.pr), 55, t) for t in (np.int32, np.uint32, np.uint64))
    ps = np.full((len(a.pr), 21), 0x5A5A5A5A, np.uint32)
    pts = np.full((len(a.out), 3), 9.0, np.float32)
    cs = (amd.Camera * len(cams))(*[amd.Camera.of(k) for k in cams])
    status = amd.lib().akz_match_features_seeded_pose_pairs(
        *a.head[:3], C.cast(cs, C.c_void_p) if cameras else None, *a.head[3:], C.byref(opt) if opt is not None else None, cross, *a.tail,
        f.ctypes.data_as(C.POINTER(C.c_float)), found.ctypes.data_as(C.POINTER(C.c_int32)), it.ctypes.data_as(C.POINTER(C.c_uint32)),
        run.ctypes.data_as(C.POINTER(C.c_uint64)), ps.ctypes.data_as(C.c_void_p) if poses else None, pts.ctypes.data_as(C.POINTER(C.c_float)))
    return status, a, f, found, it, run, ps, pts


def test_kept_lists_that_shrink_stay_in_their_room(ctx, amd, world, raw_lists):
    """Kind 1 at epsilon 4: the host statement says pair 3 (255 matches) loses none to the cheirality filter and its neighbour pair
    4 (256 matches) loses some.  Behind every pair's kept records its room in `out` and in `points` is untouched, and every list is
    the host's: nothing spilt into a neighbour's room."""
    feats, cams, pairs = world
    opt = options(amd, 1, 0)
    exp = [host_composite(amd, feats[a], feats[b], cams[a], cams[b], raw_lists[0][p], opt, BASE + p) for p, (a, b) in enumerate(pairs)]
    before = [len(amd.remove_outliers_seeded(feats[a][0], feats[b][0], raw_lists[0][p], opt, stream=BASE + p)[0]) for p, (a, b) in enumerate(pairs)]
    assert len(exp[3][0]) == before[3] > 100 and 0 < len(exp[4][0]) < before[4], (before[3:5], len(exp[3][0]), len(exp[4][0]))
    status, a, f, found, it, run, ps, pts = raw_call(ctx, amd, feats, cams, pairs, opt)
    assert status == 0
    at = 0
    for p, rows in enumerate(a.rows):
        n = int(a.n[p])
        assert n == len(exp[p][0]) and np.array_equal(a.out[at:at + n], exp[p][0]), p
        assert np.all(a.out["index_0"][at + n:at + rows] == 77) and np.all(a.out["distance"][at + n:at + rows] == 79.0), p
        assert np.array_equal(ps[p], exp[p][4]), p
        if exp[p][5] is not None:
            assert np.array_equal(pts[at:at + n].view(np.uint32), exp[p][5].view(np.uint32)), p
            assert np.all(pts[at + n:at + rows] == 9.0), p
        else:
            assert np.all(pts[at:at + rows] == 9.0), p     # without a pose no point is written
        at += rows


def test_refusals_come_before_any_gpu_work(ctx, amd, world):
    feats, cams, pairs = world
    good = options(amd, 3, 0)
    bad_cams = []
    for field, v in ((0, 0.0), (1, 0.0), (2, float("nan")), (3, float("inf")), (0, float("-inf"))):
        c = [list(k) for k in cams]
        c[15][field] = v          # a set no pair's first member: every camera of the n_sets is looked at
        bad_cams.append(c)
    calls = [dict(opt=None), dict(opt=good.copy(struct_size=72)), dict(opt=good.copy(model_kind=0)), dict(opt=good.copy(model_kind=2)),
             dict(opt=good.copy(guided=1, guided_radius=3.0)), dict(opt=good, cameras=False), dict(opt=good, poses=False),
             dict(opt=good, pairs=pairs + [(0, 16)])] + [dict(opt=good, cams=c) for c in bad_cams]
    before = amd.debug_resource_counts()
    for k, kw in enumerate(calls):
        status, a, f, found, it, run, ps, pts = raw_call(ctx, amd, feats, kw.get("cams", cams), kw.get("pairs", pairs), kw["opt"],
                                                         cameras=kw.get("cameras", True), poses=kw.get("poses", True))
        assert status == -1, k
        assert np.all(a.out["index_0"] == 77) and np.all(a.n == 12345) and np.all(f == 7.0), k    # nothing was written
        assert np.all(found == 55) and np.all(it == 55) and np.all(run == 55) and np.all(ps == 0x5A5A5A5A) and np.all(pts == 9.0), k
    assert amd.debug_resource_counts() == before          # nothing was allocated: the refusals come before any GPU work
    with pytest.raises(amd.AkazeError):
        ctx.match_features_seeded_pose_pairs(feats, cams, pairs, good.copy(guided=1))
    # NULL points and NULL model .. trials_run are allowed
    a = amd._PairsArgs(ctx, feats, pairs[:2])
    cs = (amd.Camera * len(cams))(*[amd.Camera.of(k) for k in cams])
    ps = (amd.Pose * 2)()
    assert amd.lib().akz_match_features_seeded_pose_pairs(*a.head[:3], C.cast(cs, C.c_void_p), *a.head[3:], C.byref(good), 0, *a.tail, None, None,
                                                          None, None, C.cast(ps, C.c_void_p), None) == 0
    assert ps[1].found == 1 and int(a.n[1]) == ps[1].in_front[ps[1].winner]


def test_the_plain_call_is_unchanged(ctx, amd, world):
    """akz_match_features_seeded_pairs before and after a pose call on the same context: identical bytes; the scratch audit is
    clean after the pose call."""
    feats, cams, pairs = world
    opt = options(amd, 3, 2)

    def plain():
        res = ctx.match_features_seeded_pairs(feats, pairs, opt)
        return [(m.tobytes(), None if h is None else np.asarray(h, np.float32).tobytes(), it, tr) for m, h, it, tr in res]
    first = plain()
    posed = ctx.match_features_seeded_pose_pairs(feats, cams, pairs, opt, points=True)
    bad = [r for r in ctx.debug_audit_scratch() if r["first_bad"] is not None]
    assert not bad, bad
    assert plain() == first
    # and the pose call's model, found, fits and trials are the plain call's: the stage changes the list alone
    for p, (g, e) in enumerate(zip(posed, first)):
        assert (None if g[1] is None else np.asarray(g[1], np.float32).tobytes(), g[2], g[3]) == e[1:], p
