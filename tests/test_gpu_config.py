"""Whole extractions across the accepted Config space against the oracle: configs that put detector sigma 1 to 6 on the
levels (5 and 6: the two-kernel detector and the stand-alone NMS, and on the coarse stream the reversed join), level-0 blurs of
3 to 13 taps (only 5 fits k_head and the blur5 march), FED schedules up to 98 steps per level, 32 and 4 levels, and contrast
percentiles / bin counts at their edges -- each under every forced gate side of tests/test_gpu_gates.py, through both entry
points, u8 and f32 input, batches of different frames.  Then the contrast scratch of one context through a sequence of jobs
whose histogram size grows and shrinks, checked against a float64 restatement of compute_contrast_factor."""
import math

import numpy as np
import pytest

from test_gpu_extract import assert_same_result

pytestmark = pytest.mark.gpu

FRAME_W, FRAME_H = 640, 480

# (name, Config overrides, what tests/test_config_space.py checks the plan of a 640 x 480 frame reaches)
CONFIGS = [
    ("base0.9", dict(base_scale_offset=0.9), dict(taps=3, sigmas=[1, 2], steps=(2, 16))),
    ("base1.0_deriv0.6", dict(base_scale_offset=1.0, derivative_factor=0.6), dict(taps=3, sigmas=[1], steps=(2, 18))),
    ("deriv2.3", dict(derivative_factor=2.3), dict(taps=5, sigmas=[4, 5, 6], steps=(3, 29))),
    ("base2.5", dict(base_scale_offset=2.5), dict(taps=7, sigmas=[4, 5, 6], steps=(4, 45))),
    ("base4.0_deriv0.75", dict(base_scale_offset=4.0, derivative_factor=0.75), dict(taps=9, sigmas=[3, 4, 5], steps=(6, 71))),
    ("base4.8_deriv0.6", dict(base_scale_offset=4.8, derivative_factor=0.6), dict(taps=11, sigmas=[3, 4, 5], steps=(8, 86))),
    ("base5.5_deriv0.5", dict(base_scale_offset=5.5, derivative_factor=0.5), dict(taps=13, sigmas=[3, 4, 5], steps=(9, 98))),
    ("sub8_oct8", dict(num_sublevels=8, max_octave_evolution=8), dict(taps=5, sigmas=[2, 3, 4], levels=32)),
    ("sub1_oct8", dict(num_sublevels=1, max_octave_evolution=8), dict(taps=5, sigmas=[2], levels=4)),
]
# the percentile / bin count edges: 0 (contrast 0: NaN planes), 1, +inf (the saturating threshold: 0.03); 1 bin, 641 (past
# the 640 of the march / stream contrast kernels), 4096 (the most k_head's histogram pass takes)
CONTRAST_CONFIGS = [
    ("pct0", dict(contrast_percentile=0.0), None),
    ("pct1", dict(contrast_percentile=1.0), None),
    ("pct_inf", dict(contrast_percentile=math.inf), None),
    ("bins1", dict(contrast_factor_num_bins=1), None),
    ("bins641", dict(contrast_factor_num_bins=641), None),
    ("bins4096_pct0.93", dict(contrast_factor_num_bins=4096, contrast_percentile=0.93), None),
]


def unit(frames):
    """u8 -> f32 in [0, 1] as image.rs:136 converts it (the oracle's result for the u8 frame is the f32 frame's too)"""
    return (frames.astype(np.float32) * np.float32(1.0)) / np.float32(255.0)


def check_kernel_rows(label, rows, sigmas):
    """What the forced row of test_gpu_gates.FORCED must have run, from akz_debug_kernel_rows."""
    kinds = {}
    for r in rows:
        kinds.setdefault(r["kind"], set()).add(r["param"])
    small = {s for s in sigmas if s <= 4}
    for k in (4, 5):  # the one-kernel detectors stop at sigma 4: levels of sigma 5 / 6 never reach them
        assert kinds.get(k, set()) <= small, (label, k, kinds.get(k))
    if "marches wherever supported" in label:
        assert 4 not in kinds and 1 in kinds, (label, kinds)
        assert not small or 5 in kinds, (label, kinds)
    elif "march_px: tiled detector" in label:
        assert 5 not in kinds and kinds.get(4, set()) == small, (label, kinds)
    elif "tiled detector pair" in label:
        assert 4 not in kinds and 5 not in kinds, (label, kinds)
    elif "one launch per step" in label:  # (its launches are recorded under the k_fed_own row)
        assert not ({1, 3} & set(kinds)), (label, kinds)
    assert {1, 2, 3} & set(kinds), (label, kinds)  # some FED family recorded its steps


@pytest.mark.parametrize("case", CONFIGS + CONTRAST_CONFIGS, ids=[c[0] for c in CONFIGS + CONTRAST_CONFIGS])
def test_config_under_every_forced_row(ctx, amd, ref, case):
    import torch
    from test_gpu_gates import FORCED
    name, kw, _ = case
    cfg = amd.Config(**kw)
    sigmas = {lv["det_sigma"] for lv in amd.plan_levels(FRAME_W, FRAME_H, cfg)}
    frames = np.stack([amd.synth_frame(FRAME_W, FRAME_H, 300 + 7 * i) for i in range(3)])
    rfs = [ref.extract(frames[i], ref.default_config(**kw), threads=8) for i in range(3)]
    nan = any(r.contrast == 0.0 for r in rfs)
    d_u8 = torch.from_numpy(frames).cuda()
    d_f32 = torch.from_numpy(unit(frames)).cuda()
    torch.cuda.synchronize()
    try:
        for label, force, undo in FORCED:
            force(ctx)
            try:
                sync = ctx.extract_features(d_u8, cfg, keep_all_planes=True)
                for i in range(3):
                    assert_same_result(sync, rfs[i], planes=(i == 2), img=i, equal_nan=nan)
                sync.close()
                asyn = ctx.extract_begin(d_f32, cfg, keep_all_planes=True).finish()
                for i in range(3):
                    assert_same_result(asyn, rfs[i], planes=(i == 0), img=i, equal_nan=nan)
                asyn.close()
                ctx.set_profiling(1)
                ctx.kernel_rows(reset=True)
                prof = ctx.extract_features(d_u8, cfg, keep_all_planes=True)
                rows = ctx.kernel_rows(reset=True)
                ctx.set_profiling(0)
                assert prof.keypoints(1).tobytes() == rfs[1].keypoints().tobytes(), (name, label)
                prof.close()
                check_kernel_rows(label, rows, sigmas)
            finally:
                ctx.set_profiling(0)
                undo(ctx)
    finally:
        for _, _, undo in FORCED:
            undo(ctx)
        for r in rfs:
            r.close()


@pytest.mark.parametrize("kw", [dict(derivative_factor=2.3), dict(base_scale_offset=2.5)], ids=["deriv2.3", "base2.5"])
def test_sigma56_lean_jobs_in_flight(amd, ref, kw):
    """Detector sigma 5 / 6 in lean jobs (keep_all_planes=False) on the batch path, three jobs in flight: the two-kernel
    detector writes its second derivatives nowhere, and where the coarse chain has such levels the main stream joins it."""
    import torch
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    c.debug_set_schedule(4, 1)
    try:
        cfg = amd.Config(**kw)
        batches = [np.stack([amd.synth_frame(FRAME_W, FRAME_H, 400 + 3 * b + i) for i in range(3)]) for b in range(3)]
        dev = [torch.from_numpy(b).cuda() for b in batches]
        torch.cuda.synchronize()
        jobs = [c.extract_begin(d, cfg, keep_all_planes=False) for d in dev]
        res = [j.finish() for j in jobs]
        for b in range(3):
            for i in range(3):
                rf = ref.extract(batches[b][i], ref.default_config(**kw), threads=8)
                assert rf.num_keypoints > 0
                assert_same_result(res[b], rf, planes=(b == 1 and i == 2), img=i)
                rf.close()
            res[b].close()
    finally:
        c.close()


def test_sigma56_lone_1080p_default_gates(ctx, amd, ref):
    """A lone 1080p frame whose levels take detector sigma 4, 5 and 6, under the default gates: every plane against the oracle."""
    kw = dict(derivative_factor=2.3)
    frame = amd.synth_frame(1920, 1080, 77)
    rf = ref.extract(frame, ref.default_config(**kw), threads=8)
    assert rf.num_keypoints > 100
    assert_same_result(ctx.extract_features(frame, amd.Config(**kw)), rf)
    rf.close()


@pytest.mark.parametrize("prep_mode", [0, 3, 1], ids=["fused_head", "march", "stream"])
def test_contrast_scratch_through_a_sequence_of_jobs(amd, ref, prep_mode):
    """One fresh context, jobs whose contrast scratch alternately grows and shrinks -- (6 frames, few bins) and (1 frame,
    4096 bins) -- at percentiles on and off bin edges and at the saturating ones: each job's contrast factor equals the float64
    restatement of compute_contrast_factor (tests/test_config_space.py) on the oracle's Lt0.  Under prep mode 0 these small jobs
    take k_head + k_contrast_hist_final, which leaves the scratch zero behind itself for the next job (no clearing launch); under
    3 / 1 the march / stream contrast passes up to 640 bins."""
    import torch
    from test_config_space import PERCENTILE_EXTRAS, contrast_from_histogram, gradient_histogram, percentile_for, u8_unit
    w, h = 320, 240
    frames = np.stack([amd.synth_frame(w, h, 500 + i) for i in range(6)])
    lt0 = [ref.gaussian_blur(u8_unit(f), 1.6) for f in frames]
    pairs = []
    for img in lt0:
        b = ref.gaussian_blur(img, 1.0)
        pairs.append((ref.scharr(b, True, False, 1), ref.scharr(b, False, True, 1)))
    hists = {}

    def hist(i, nbins):
        if (i, nbins) not in hists:
            hists[(i, nbins)] = gradient_histogram(*pairs[i], nbins)
        return hists[(i, nbins)]

    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    c.set_prep_mode(prep_mode)
    d6 = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    try:
        rng = np.random.default_rng(prep_mode)
        jobs = 0
        for step, pct in enumerate(PERCENTILE_EXTRAS + [None] * 6):
            for n, nbins in ((6, (1, 2, 3, 7, 300, 640)[step % 6]), (1, 4096)):
                i0 = step % 6 if n == 1 else 0
                if pct is None:  # a percentile exactly at the cumulative count of some bin of the first image
                    hm, hs, npts = hist(i0, nbins)
                    cum = np.cumsum(hs)
                    p = percentile_for(npts, int(cum[rng.integers(0, nbins)]) + int(rng.integers(0, 2)))
                else:
                    p = pct
                cfg = amd.Config(contrast_factor_num_bins=nbins, contrast_percentile=p)
                res = c.extract_features(d6[i0:i0 + n], cfg, keep_all_planes=False)
                for i in range(n):
                    want = contrast_from_histogram(*hist(i0 + i, nbins), p)
                    assert res.contrast(i) == want, (prep_mode, jobs, n, nbins, p, i, res.contrast(i), want)
                res.close()
                jobs += 1
        assert jobs == 30
    finally:
        c.close()
