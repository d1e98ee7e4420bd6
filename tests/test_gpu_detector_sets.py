"""k_detector_march over a SET of levels (one launch per sigma_size, width parity and kept planes; csrc/akz_march.hip,
det_set_cell): whole extractions at the smallest shapes at which the set prologue -- workgroup -> (entry, image, band, strip)
-- can go wrong, each through extract_features and extract_begin(...).finish() with every plane kept, against the oracle
(all planes as bytes, keypoints, descriptor rows) with the detectors launched per set, per level (debug_set_schedule(11, 1))
and as the default has them."""
import numpy as np
import pytest

from test_gpu_extract import assert_same_result

pytestmark = pytest.mark.gpu

# (id, frames, w, h, Config overrides, detector mode, extra schedule (key, value) or None)
CASES = [
    # full resolution odd, half resolution (48 x 37) even: sets split by parity; at 24 x 18 sigma 2 marches while sigma 3 and 4
    # have no march: sets next to tiled levels; three images, one strip
    ("3x97x75", 3, 97, 75, {}, 5, None),
    # two strips at full resolution, one at half; 125 x 32 is odd: entries differ in strips, bands and images per cell
    ("2x500x130", 2, 500, 130, {}, 5, None),
    # three strips; at 482 x 34 the second strip is two columns wide; one band per level: most of every entry's 8 cells are padding
    ("1x964x68", 1, 964, 68, {}, 5, None),
    # more than four levels of one sigma_size: a group is split at the cap
    ("3x97x75_sub5_oct5", 3, 97, 75, dict(num_sublevels=5, max_octave_evolution=5), 5, None),
    # the batch path as the headline runs it: forked coarse chain, full-resolution levels in sets on the main stream ...
    ("2x640x480_default", 2, 640, 480, {}, None, None),
    # ... and cut into 16-row bands: many cells per entry
    ("2x640x480_rows16", 2, 640, 480, {}, None, (7, 16)),
]


def march_launches(ctx, dev, cfg):
    """(launches, levels' pixels) of k_detector_march in one extraction through the begin / finish interface (whose job gate
    the default-mode cases rely on), from akz_debug_kernel_rows"""
    ctx.set_profiling(1)
    try:
        ctx.kernel_rows(reset=True)
        ctx.extract_begin(dev, cfg, keep_all_planes=True).finish().close()
        rows = [r for r in ctx.kernel_rows(reset=True) if r["kind"] == 5]
    finally:
        ctx.set_profiling(0)
    return sum(r["launches"] for r in rows), sum(r["px"] for r in rows)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_detector_sets_match_oracle(ctx, amd, ref, case):
    import torch
    name, n, w, h, kw, det_mode, extra = case
    cfg = amd.Config(**kw)
    frames = np.stack([amd.synth_frame(w, h, 900 + 5 * i) for i in range(n)])
    rfs = [ref.extract(frames[i], ref.default_config(**kw), threads=8) for i in range(n)]
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    launches = {}
    try:
        if det_mode is not None:
            ctx.set_detector_mode(det_mode)
        if extra:
            ctx.debug_set_schedule(*extra)
        for sched in (2, 1, 0):  # sets, one launch per level (the reference schedule), the default
            ctx.debug_set_schedule(11, sched)
            if det_mode is not None:
                sync = ctx.extract_features(dev, cfg, keep_all_planes=True)
                for i in range(n):
                    assert_same_result(sync, rfs[i], planes=True, img=i)
                sync.close()
            asyn = ctx.extract_begin(dev, cfg, keep_all_planes=True).finish()
            for i in range(n):
                assert_same_result(asyn, rfs[i], planes=True, img=i)
            asyn.close()
            launches[sched] = march_launches(ctx, dev, cfg)
        # the same levels' pixels went through the march either way, in fewer launches when they are sets
        assert launches[2][1] == launches[1][1] > 0, (name, launches)
        assert launches[2][0] < launches[1][0], (name, launches)
        assert launches[0] in (launches[1], launches[2]), (name, launches)
    finally:
        ctx.set_profiling(0)
        ctx.debug_set_schedule(11, 0)
        if extra:
            ctx.debug_set_schedule(extra[0], 0)
        ctx.set_detector_mode(2)
        for r in rfs:
            r.close()
