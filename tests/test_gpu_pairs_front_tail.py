"""What the RANSAC pairs calls share (pairs_front, pairs_tail: akz_match_api.cpp) where the other files do not pin it.  Mixed
found flags under the guided stage: a pair without a model between two pairs with one, and a pair whose second set is empty -- the
read-back of the guided lists spans up to the LAST pair with a model, and the copy-out picks per pair between the guided and the
filtered list; the batch equals the loop of one-pair calls for the call that draws on the host and for the seeded call, with and
without the stopping rule.  The timed call (akz_debug_match_pairs_split): the same outputs as the untimed one for the host-draw
call, the seeded call and the seeded cross call, six finite intervals, the trials' interval above zero, and switching it off
restores the untimed path.  No thresholds on the times."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_homography_refit import _same3
from test_gpu_match_pairs import _color
from test_seeded_ransac_host import options, same4

pytestmark = pytest.mark.gpu

N, NB, RATIO, EPS, TRIALS, ITS, RADIUS = 300, 61, 0.86, 3.0, 300, 2, 3.0
SHIFT = (5.0, 3.0)
# (related, unrelated, related), then an empty second set
PAIRS = [(0, 1), (0, 2), (1, 0), (0, 3)]
FOUND = [True, False, True, False]


def build_sets(amd):
    """sets 0 / 1: N keypoints related by SHIFT (+ N(0, 0.5); three in ten displaced by 50 .. 400 px) through equal random rows in
    another order; set 2: N random points with N random rows, three of them rows of set 0 -- three matches, fewer than a sample, so
    the pair has a filtered list to hand back and no model; set 3: empty"""
    rng = np.random.default_rng(1905)

    def keypoints(xy):
        k = np.zeros(len(xy), amd.KEYPOINT_DTYPE)
        k["x"], k["y"] = xy[:, 0], xy[:, 1]
        return k

    p0 = rng.uniform((50, 50), (1800, 1000), (N, 2))
    out = rng.uniform(size=N) < 0.3
    p1 = p0 + SHIFT + rng.normal(0, 0.5, (N, 2)) * (~out)[:, None]
    ang, dist = rng.uniform(0, 2 * np.pi, N), rng.uniform(50, 400, N)
    p1[out] += (np.c_[np.cos(ang), np.sin(ang)] * dist[:, None])[out]
    perm = rng.permutation(N)
    d0 = rng.integers(0, 256, (N, NB), dtype=np.uint8)
    d1, q1 = np.zeros_like(d0), np.zeros_like(p1)
    d1[perm], q1[perm] = d0, p1
    d2 = rng.integers(0, 256, (N, NB), dtype=np.uint8)
    d2[[7, 150, 299]] = d0[[250, 3, 100]]
    return [(keypoints(p0), d0), (keypoints(q1), d1), (keypoints(rng.uniform((0, 0), (1920, 1080), (N, 2))), d2),
            (np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, NB), np.uint8))]


def seeded_options(amd, conf, **kw):
    return options(amd, "H", max_trials=TRIALS, confidence=conf, refine_iterations=ITS, stream_base=(1 << 64) - 2, lowes_ratio=RATIO,
                   epsilon_inliers=EPS, **kw)


@pytest.fixture(scope="module")
def sets(amd):
    return build_sets(amd)


@pytest.fixture(scope="module")
def raws(ctx, sets):
    """every pair's raw list (computed once, left unchanged)"""
    return [ctx.descriptor_match(sets[a][1], sets[b][1], 10000, RATIO) for a, b in PAIRS]


def test_the_case_is_mixed(amd, sets, raws):
    """the host statements on the raw lists: the related pairs have a model, the unrelated one and the empty one have none"""
    assert len(raws[0]) == N and len(raws[2]) == N and len(raws[1]) == 3 and len(raws[3]) == 0
    amd.random_seed(42, 69)
    host = [amd.remove_outliers_homography(sets[a][0], sets[b][0], raw, TRIALS, amd.HOMOGRAPHY_EPSILON_MODEL, EPS)[1]
            for (a, b), raw in zip(PAIRS, raws)]
    assert [h is not None for h in host] == FOUND
    for conf in (0.0, 0.99):
        opt = seeded_options(amd, conf)
        got = [amd.remove_outliers_seeded(sets[a][0], sets[b][0], raw, opt, stream=(opt.stream_base + p) & ((1 << 64) - 1))
               for p, ((a, b), raw) in enumerate(zip(PAIRS, raws))]
        assert [g[1] is not None for g in got] == FOUND, conf


def test_host_draw_guided_batch_equals_the_loop(ctx, amd, sets):
    amd.random_seed(42, 69)
    got = ctx.match_features_homography_refined_guided_pairs(sets, PAIRS, RATIO, TRIALS, EPS, ITS, RADIUS, RATIO)
    after_batch = _color(amd)
    amd.random_seed(42, 69)
    exp = [amd.match_features_homography_refined_guided(sets[a][0], sets[a][1], sets[b][0], sets[b][1], RATIO, TRIALS, EPS, ITS, RADIUS,
                                                        RATIO, ctx=ctx) for a, b in PAIRS]
    assert after_batch == _color(amd)
    assert [g[1] is not None for g in got] == FOUND
    for p, (g, e) in enumerate(zip(got, exp)):
        _same3(g, e, (p, PAIRS[p]))
    # found: the guided list, which the planted scene fills (span = the third pair's place + its count); not found: the filtered one
    assert len(got[0][0]) > N // 2 and len(got[2][0]) > N // 2 and len(got[3][0]) == 0
    plain = ctx.match_features_homography_refined_pairs(sets, PAIRS, RATIO, TRIALS, EPS, ITS)
    assert np.array_equal(got[1][0], plain[1][0]) and len(got[1][0]) == 3


@pytest.mark.parametrize("conf", [0.0, 0.99])
def test_seeded_guided_batch_equals_the_loop(ctx, amd, sets, conf):
    opt = seeded_options(amd, conf, guided=1, guided_radius=RADIUS, guided_lowes_ratio=RATIO)
    got = ctx.match_features_seeded_pairs(sets, PAIRS, opt)
    assert [g[1] is not None for g in got] == FOUND
    for p, (a, b) in enumerate(PAIRS):
        one = opt.copy(stream_base=(opt.stream_base + p) & ((1 << 64) - 1))     # (the stream wraps as u64)
        same4(got[p], ctx.match_features_seeded_pairs([sets[a], sets[b]], [(0, 1)], one)[0], ("loop", p))
    assert len(got[0][0]) > N // 2 and len(got[2][0]) > N // 2 and len(got[1][0]) == 3 and len(got[3][0]) == 0
    assert got[1][3] == 0 and got[3][3] == 0 and got[0][3] > 0 and got[2][3] > 0
    if conf == 0.0:
        assert got[0][3] == TRIALS and got[2][3] == TRIALS


def _split(ctx, amd, enable):
    ms = (C.c_double * 6)()
    assert amd.lib().akz_debug_match_pairs_split(ctx._h, enable, ms) == 0
    return list(ms)


@pytest.mark.parametrize("call", ["host_draw", "seeded", "seeded_cross"])
def test_the_timed_call_gives_the_untimed_outputs(ctx, amd, sets, call):
    opt = seeded_options(amd, 0.99, guided=1, guided_radius=RADIUS, guided_lowes_ratio=RATIO)

    def run():
        amd.random_seed(42, 69)
        if call == "host_draw":
            return [(m, h, it, 0) for m, h, it in
                    ctx.match_features_homography_refined_guided_pairs(sets, PAIRS, RATIO, TRIALS, EPS, ITS, RADIUS, RATIO)]
        return ctx.match_features_seeded_pairs(sets, PAIRS, opt, cross_check=call == "seeded_cross")

    try:
        _split(ctx, amd, 0)
        untimed = run()
        _split(ctx, amd, 1)
        timed = run()
        ms = _split(ctx, amd, 0)            # the timed call's intervals; off again
        again = run()
        assert _split(ctx, amd, 0) == ms    # the untimed path: it leaves the intervals alone
    finally:
        _split(ctx, amd, 0)
    assert [g[1] is not None for g in untimed] == FOUND
    for p, (u, t, a) in enumerate(zip(untimed, timed, again)):
        same4(t, u, ("timed", call, p))
        same4(a, u, ("off again", call, p))
    assert all(math.isfinite(v) and v >= 0.0 for v in ms), ms
    assert ms[3] > 0.0, ms                  # two pairs ran trials / rounds
