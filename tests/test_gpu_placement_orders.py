"""Two placement orders over one layout (SetsBlock, akz_pairs_layout.hpp): a sets call places the sets its pairs name in order of
first use, a bank places every set in index order.  Four sets of 70, 0, 70 and 33 rows and the pairs (2, 0), (3, 2), (2, 1): first
use is 2, 0, 3, 1 -- sets 0 and 2 change places against the bank, and set 1 is empty.  The sets call, the bank call and the loop
of one-pair calls must agree bit for bit, over the multi-set scan (61-byte rows) and the pair matcher (64-byte rows), for the seeded
call with and without the guided stage and for the call that draws on the host."""
import numpy as np
import pytest

from test_gpu_fundamental_refit import _same3
from test_seeded_ransac_host import same4

pytestmark = pytest.mark.gpu

SIZES = (70, 0, 70, 33)
PAIRS = [(2, 0), (3, 2), (2, 1)]
FOUND = [True, False, False]
RATIO, TRIALS, ITS, RADIUS = 0.86, 300, 2, 3.0
SHIFT = (5.0, 3.0)


def build_sets(amd, nb):
    """sets 0 / 2: 70 keypoints related by SHIFT (+ N(0, 0.5); three in ten displaced by 50 .. 400 px) through equal random rows in
    another order; set 3: 33 random points with random rows, three of them rows of set 2 -- three matches, fewer than a sample; set 1:
    empty (test_gpu_pairs_front_tail.build_sets at these sizes)"""
    rng = np.random.default_rng(1905)
    n = SIZES[0]

    def keypoints(xy):
        k = np.zeros(len(xy), amd.KEYPOINT_DTYPE)
        k["x"], k["y"] = xy[:, 0], xy[:, 1]
        return k

    p0 = rng.uniform((50, 50), (1800, 1000), (n, 2))
    out = rng.uniform(size=n) < 0.3
    p2 = p0 + SHIFT + rng.normal(0, 0.5, (n, 2)) * (~out)[:, None]
    ang, dist = rng.uniform(0, 2 * np.pi, n), rng.uniform(50, 400, n)
    p2[out] += (np.c_[np.cos(ang), np.sin(ang)] * dist[:, None])[out]
    perm = rng.permutation(n)
    d0 = rng.integers(0, 256, (n, nb), dtype=np.uint8)
    d2, q2 = np.zeros_like(d0), np.zeros_like(p2)
    d2[perm], q2[perm] = d0, p2
    d3 = rng.integers(0, 256, (SIZES[3], nb), dtype=np.uint8)
    d3[[7, 15, 32]] = d2[[60, 3, 41]]
    sets = [(keypoints(p0), d0), (np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, nb), np.uint8)), (keypoints(q2), d2),
            (keypoints(rng.uniform((0, 0), (1920, 1080), (SIZES[3], 2))), d3)]
    assert tuple(len(d) for _, d in sets) == SIZES
    return sets


@pytest.mark.parametrize("guided", [0, 1])
@pytest.mark.parametrize("nb", [61, 64])
def test_seeded_sets_call_bank_call_and_loop_agree(ctx, amd, nb, guided):
    sets = build_sets(amd, nb)
    opt = amd.RansacOptions(model_kind=amd.RANSAC_FUNDAMENTAL_NORMALISED, max_trials=TRIALS, confidence=0.99, refine_iterations=ITS,
                            epsilon_inliers=2.0, lowes_ratio=RATIO, stream_base=(1 << 64) - 2, guided=guided, guided_radius=RADIUS,
                            guided_lowes_ratio=RATIO)
    got = ctx.match_features_seeded_pairs(sets, PAIRS, opt)
    assert [g[1] is not None for g in got] == FOUND        # not vacuous: a pair with a model, pairs without
    assert len(got[0][0]) > SIZES[0] // 2 and len(got[1][0]) == 3 and len(got[2][0]) == 0
    bank = ctx.feature_bank(sets)
    try:
        assert [s["row0"] for s in bank.info()["sets"]] == [0, 70, 70, 140]   # (first use puts them at rows 70, 173, 0, 140)
        banked = ctx.match_features_seeded_pairs(bank, PAIRS, opt)
    finally:
        bank.close()
    for p, (a, b) in enumerate(PAIRS):
        same4(banked[p], got[p], ("bank", nb, guided, p))
        one = opt.copy(stream_base=(opt.stream_base + p) & ((1 << 64) - 1))     # (the stream wraps as u64)
        same4(ctx.match_features_seeded_pairs([sets[a], sets[b]], [(0, 1)], one)[0], got[p], ("loop", nb, guided, p))


@pytest.mark.parametrize("nb", [61, 64])
def test_host_draw_sets_call_equals_the_loop(ctx, amd, nb):
    sets = build_sets(amd, nb)
    amd.random_seed(42, 69)
    got = ctx.match_features_fundamental_refined_guided_pairs(sets, PAIRS, RATIO, TRIALS, 0.02, ITS, RADIUS, RATIO)
    amd.random_seed(42, 69)
    exp = [amd.match_features_fundamental_refined_guided(sets[a][0], sets[a][1], sets[b][0], sets[b][1], RATIO, TRIALS, 0.02, ITS, RADIUS,
                                                         RATIO, ctx=ctx) for a, b in PAIRS]
    assert [g[1] is not None for g in got] == FOUND
    for p, (g, e) in enumerate(zip(got, exp)):
        _same3(g, e, (nb, p, PAIRS[p]))
