"""Keypoint detection on the GPU at the edges where its copies can be wrong: the strict 4-neighbour maximum and threshold
(k_nms; tile_extrema and the fused test of k_detector_march), `dist <= size * size`, "a strictly larger response replaces",
the order-dependent rules of the cache walk, and the refinement's gate -- in the host's grid selection, the host's selection
from the device's neighbour lists, and the device's own selection (k_relations, k_sel_prepare, k_select).

1. The crafted Ldet pyramids of tests/extrema_cases.py go through akz_extract_from_planes (k_nms on the caller's Ldet, then the
   ordinary finish half) under every selection (akz_debug_set_select 0 / 1 / 2) and sort (akz_debug_set_host_sort) and through
   the overflow retry (set_candidate_hint(16)), and must equal the numpy statement (tests/extrema_numpy.py) bit for bit; angles
   and descriptor rows must equal tests/mldb_numpy.py on the same random Lt / Lx / Ly.  tests/test_extrema_host.py shows on the
   CPU that these pyramids tell every flipped comparison from the right one.  The result does not expose the extrema count
   (before the refinement); the host test checks it through akz_host_select_keypoints.
2. The fused emitters cannot be fed a crafted Ldet: a small batch is extracted with detector_threshold set to an Ldet value
   that IS a strict local maximum (a survivor's response), and to the float32 just below it.  The oracle alone shows that the
   keypoint goes and stays; every detector mode must agree with the oracle at both.

akz_extract_from_planes takes ONE image: the per-image runs of a batch's selection stay with the random-job tests of
tests/test_gpu_extract.py (test_selection_on_the_device, test_selection_from_device_neighbour_lists)."""
import functools

import numpy as np
import pytest

import extrema_cases as X
import extrema_numpy as E
from test_gpu_detector_sets import CASES as DETECTOR_SET_CASES
from test_gpu_extract import assert_same_result

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "response", "size", "octave", "class_id", "angle")
DEFAULT_HINT = 1 << 15  # akz_ctx's initial candidate room


@functools.lru_cache(maxsize=None)
def expected(name):
    """the case's planes, and what the two statements say: keypoints with angle, descriptor rows"""
    import mldb_numpy as M
    w, h, cfg, levels, ldets = X.pyramid(X.CASE_FN[name]())
    aux = X.aux_planes(levels, 11)
    planes = [dict(aux[l], Ldet=ldets[l]) for l in range(len(levels))]
    kps, _ = E.detect(ldets, levels, cfg)
    ang, desc, _ = M.describe([(a["Lt"], a["Lx"], a["Ly"]) for a in aux], [lv[2] for lv in levels], kps, 3, "clamped")
    kps = kps.copy()
    kps["angle"] = ang
    return w, h, {k: getattr(cfg, k) for k in X.DEFAULTS}, planes, kps, desc


def assert_case(res, name):
    _, _, _, planes, kps, desc = expected(name)
    got = res.keypoints()
    assert res.counts() == (len(planes), len(kps), 61), (name, res.counts(), len(kps))
    for f in FIELDS:
        ga, ea = np.asarray(got[f]), np.asarray(kps[f])
        if ga.dtype.kind == "f":
            ga, ea = ga.view(np.uint32), ea.view(np.uint32)
        assert np.array_equal(ga, ea), (name, f, np.nonzero(ga != ea)[0][:5])
    assert np.array_equal(res.descriptors(), desc), name


@pytest.mark.parametrize("host_sort", [True, False], ids=["hostsort", "devsort"])
@pytest.mark.parametrize("select", [0, 1, 2], ids=["grids", "lists", "device"])
@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_crafted_pyramids_all_selections(ctx, amd, name, select, host_sort):
    w, h, over, planes, _, _ = expected(name)
    try:
        ctx.debug_set_select(select)
        ctx.debug_set_host_sort(host_sort)
        res = ctx.extract_from_planes(w, h, planes, amd.Config(**over))
        info = ctx.debug_select_info()
    finally:
        ctx.debug_set_select(None)
        ctx.debug_set_host_sort(None)
    print(f"{name} select={select} host_sort={host_sort}: select_info {info[:4]}")
    assert_case(res, name)
    res.close()
    if select == 2 and name.startswith("dense"):
        # more earlier neighbours than a list holds, more members than a reverse list keeps: handed back to the host
        assert info[0] != 2 and (info[2] & 0xffff) == 1, (name, info)
    elif select == 2:  # (the device's selection takes the device's sort whatever the sort hook says: host_sort is inert here)
        assert info[0] == 2 and info[2] == 0, (name, info)
    elif select == 1:  # (the lists need the device's sort: with the host's sort forced the job takes the grids, as under select 0)
        assert info[0] == (0 if host_sort else 1), (name, info)
    else:
        assert info[0] == 0, (name, info)


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_crafted_pyramids_overflow_retry(ctx, amd, name):
    """Room for 16 candidates, the smallest list there is: every case has more (the fillers of extrema_cases.Planes.fill see
    to it; tests/test_extrema_host.py counts them), so k_nms runs a second time on the stored Ldet planes with room, and the
    host sorts and selects that list.  The hooks are at their defaults.  (The jobs of `dense`'s shape find the device's
    selection switched off for a few jobs after its hand-back above, which is why that case has a shape of its own; the
    retry goes to the host's selection either way.)"""
    w, h, over, planes, _, _ = expected(name)
    try:
        ctx.set_candidate_hint(16)
        res = ctx.extract_from_planes(w, h, planes, amd.Config(**over))
        info = ctx.debug_select_info()
    finally:
        ctx.set_candidate_hint(DEFAULT_HINT)
    print(f"{name} hint 16: select_info {info[:4]}")
    assert_case(res, name)
    res.close()
    assert info[3] > 16 and info[0] != 2, (name, info)  # more candidates than the list held: the pass was repeated, the host selected


# ---- threshold equality through the fused emitters -------------------------------------------------------------------------
def noisy_frame(amd, w, h, i):
    """that module's frame i with seeded noise of +-24 grey levels on it: the plain synthetic frames have fewer than 20
    keypoints on level 0 at every one of its shapes (8 and 16 at 640 x 480), the noise brings fine-scale extrema"""
    noise = np.random.default_rng(100 + i).integers(-24, 25, (h, w))
    return np.clip(amd.synth_frame(w, h, 900 + 5 * i).astype(np.int32) + noise, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def threshold_jobs(amd, ref):
    """On the CPU: the smallest batch of tests/test_gpu_detector_sets.py whose first image has at least 20 keypoints on level 0
    and one on a level of octave 1 under the default Config; two of its survivors (the median response of level 0, the median
    of octave 1) and, for each, the thresholds T = its Ldet value and the float32 below T, with the oracle's results."""
    for _, n, w, h, kw, _, _ in sorted(DETECTOR_SET_CASES, key=lambda c: c[1] * c[2] * c[3]):
        if kw:
            continue
        frames = np.stack([noisy_frame(amd, w, h, i) for i in range(n)])
        first = ref.extract(frames[0])
        rk = first.keypoints()
        first.close()
        lvl0, oct1 = rk[rk["class_id"] == 0], rk[rk["octave"] == 1]
        if len(lvl0) >= 20 and len(oct1) >= 1:
            break
    else:
        raise AssertionError("no batch with 20 keypoints on level 0 and one on octave 1")
    picks = [np.sort(lvl0, order="response")[len(lvl0) // 2], np.sort(oct1, order="response")[len(oct1) // 2]]
    jobs = []
    for kp in picks:
        t = np.float32(kp["response"])
        for thr, present in ((t, False), (np.nextafter(t, np.float32(-np.inf)), True)):
            assert np.float32(float(thr)) == thr  # the reference's `as f32` gives the value back
            rfs = [ref.extract(frames[i], ref.default_config(detector_threshold=float(thr))) for i in range(n)]
            jobs.append((float(thr), rfs))
            k0 = rfs[0].keypoints()
            there = ((k0["class_id"] == kp["class_id"]) & (k0["response"] == kp["response"]) & (k0["x"] == kp["x"]) & (k0["y"] == kp["y"])).sum()
            assert there == (1 if present else 0), (kp, thr, there)  # the oracle alone: at T the keypoint is gone, below T it is there
            assert rfs[0].num_keypoints >= 1
    yield frames, jobs
    for _, rfs in jobs:
        for rf in rfs:
            rf.close()


def detector_launches(ctx, dev, cfg):
    """launches of (k_detector_tiled over a set, k_detector_march) in one extraction, from akz_debug_kernel_rows"""
    ctx.set_profiling(1)
    try:
        ctx.kernel_rows(reset=True)
        ctx.extract_begin(dev, cfg).finish().close()
        rows = ctx.kernel_rows(reset=True)
    finally:
        ctx.set_profiling(0)
    return tuple(sum(r["launches"] for r in rows if r["kind"] == kind) for kind in (4, 5))


@pytest.mark.parametrize("k", range(4), ids=["level0_at_T", "level0_below_T", "octave1_at_T", "octave1_below_T"])
def test_threshold_equality_through_the_fused_emitters(ctx, amd, threshold_jobs, k):
    import torch
    frames, jobs = threshold_jobs
    thr, rfs = jobs[k]
    cfg = amd.Config(detector_threshold=thr)
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()

    def both(what):
        for res in (ctx.extract_features(dev, cfg), ctx.extract_begin(dev, cfg).finish()):
            for i, rf in enumerate(rfs):
                assert_same_result(res, rf, planes=False, img=i)
            res.close()
        tiled, march = detector_launches(ctx, dev, cfg)
        print(f"threshold {thr!r} {what}: {[rf.num_keypoints for rf in rfs]} keypoints as the oracle; "
              f"{tiled} tiled-set and {march} march launches")
        return tiled, march

    try:
        for mode in (0, 4, 5):
            ctx.set_detector_mode(mode)
            tiled, march = both(f"detector mode {mode}")
            # mode 5: the march's fused test emitted the candidates of every level it supports; modes 0 and 4 never march:
            # tile_extrema did, under k_detector_tiled over sets of levels (mode 4) or under k_deriv2 (mode 0)
            assert (march > 0) == (mode == 5) and (tiled > 0) == (mode == 4), (mode, tiled, march)
        ctx.set_detector_mode(2)
        both("default mode")
        ctx.set_candidate_hint(16)
        res = ctx.extract_features(dev, cfg)
        ctx.set_candidate_hint(16)
        res2 = ctx.extract_begin(dev, cfg).finish()
        for r in (res, res2):
            for i, rf in enumerate(rfs):
                assert_same_result(r, rf, planes=False, img=i)
            r.close()
    finally:
        ctx.set_profiling(0)
        ctx.set_detector_mode(2)
        ctx.set_candidate_hint(DEFAULT_HINT)
