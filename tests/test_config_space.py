"""The accepted Config space, on the host: every config that the GPU tests of tests/test_gpu_config.py run reaches the kernel
branch it is there for (detector sigma, level-0 tap count, FED steps per level, histogram bins either side of the 640 of the
march / stream contrast kernels), every refused config is refused with its exact status, and the float64 restatement of
compute_contrast_factor that the GPU tests hold the kernels to agrees with the oracle.  No GPU needed."""
import math

import numpy as np
import pytest

from test_gpu_config import CONFIGS, CONTRAST_CONFIGS, FRAME_H, FRAME_W

USIZE_MAX = (1 << 64) - 1


def sat_usize(v):
    """Rust's `as usize` from an f64: NaN and negatives -> 0, 2^64 and above (+inf included) -> usize::MAX."""
    if not (v > 0.0):
        return 0
    if v >= 18446744073709551615.0:
        return USIZE_MAX
    return int(v)


def gradient_histogram(lx, ly, nbins):
    """contrast_factor.rs:24-55 in float64 on the scale-1 Scharr pair of the blurred image: (hmax, histogram, num_points)."""
    lx = lx[1:-1, 1:-1].astype(np.float64)
    ly = ly[1:-1, 1:-1].astype(np.float64)
    g = np.sqrt(lx * lx + ly * ly)
    hmax = float(g.max()) if g.size else 0.0
    g = g[g != 0.0]
    if not g.size:
        return hmax, np.zeros(nbins, np.int64), 0
    f = np.floor(float(nbins) * (g / hmax))  # finite, in [0, nbins]: saturation does not come in
    b = np.minimum(f.astype(np.int64), nbins - 1)  # bin_number == num_bins -> num_bins - 1
    return hmax, np.bincount(b, minlength=nbins).astype(np.int64), int(g.size)


def contrast_from_histogram(hmax, hist, num_points, percentile):
    """contrast_factor.rs:56-70: the percentile walk, with the saturating conversion of the threshold."""
    nbins = len(hist)
    threshold = sat_usize(float(num_points) * percentile)
    k, num_elements = 0, 0
    if threshold > 0:
        cum = np.cumsum(hist)
        k = int(np.searchsorted(cum, threshold)) + 1  # the first k with sum(hist[:k]) >= threshold
        if k > nbins:
            k, num_elements = nbins, int(cum[-1])
        else:
            num_elements = int(cum[k - 1])
    if num_elements >= threshold:
        return hmax * float(k) / float(nbins)
    return 0.03


def contrast_np(ref, img, percentile, gscale, nbins):
    """compute_contrast_factor(img, percentile, gscale, nbins) from the oracle's gaussian_blur and scharr planes."""
    blurred = ref.gaussian_blur(img, float(np.float32(gscale)))
    h = gradient_histogram(ref.scharr(blurred, True, False, 1), ref.scharr(blurred, False, True, 1), nbins)
    return contrast_from_histogram(*h, percentile)


def level0_taps(cfg):
    """gaussian_kernel_size(base_scale_offset as f32) (image.rs:341): the level-0 blur's tap count."""
    return 2 * math.ceil(float(np.float32(cfg.base_scale_offset))) + 1


@pytest.mark.parametrize("case", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_gpu_configs_reach_their_branches(amd, case):
    name, kw, want = case
    cfg = amd.Config(**kw)
    plan = amd.plan_levels(FRAME_W, FRAME_H, cfg)
    steps = [len(lv["tau"]) for lv in plan[1:]]
    got = dict(levels=len(plan), taps=level0_taps(cfg), sigmas=sorted({lv["det_sigma"] for lv in plan}),
               steps=(min(steps), max(steps)))
    for k, v in want.items():
        assert got[k] == v, (name, k, got[k], v)


def test_gpu_configs_cover_every_sigma_and_tap_count(amd):
    """Together the end-to-end configs run every detector sigma 1..6 and every level-0 blur width 3..13."""
    sigmas, taps = set(), set()
    for _, kw, _ in CONFIGS:
        cfg = amd.Config(**kw)
        sigmas |= {lv["det_sigma"] for lv in amd.plan_levels(FRAME_W, FRAME_H, cfg)}
        taps.add(level0_taps(cfg))
    assert sigmas == {1, 2, 3, 4, 5, 6}
    assert taps == {3, 5, 7, 9, 11, 13}
    # the branches behind these: the march / tiled / NMS-fused detectors stop at sigma 4; k_head and the blur5 march need 5 taps
    assert any(s > 4 for s in sigmas) and any(t not in (3, 5) for t in taps)


def test_gpu_configs_cover_every_config_field(amd):
    """Every accepted field except initial_contrast (declared, never read: evolution.rs) leaves its default in some GPU test
    of tests/test_gpu_config.py (descriptor_channels and detector_threshold: tests/test_gpu_extract.py, test_gpu_stream.py)."""
    fields = {k for _, kw, _ in CONFIGS + CONTRAST_CONFIGS for k in kw}
    want = {f for f, _ in amd.Config._fields_} - {"initial_contrast", "descriptor_channels", "descriptor_pattern_size",
                                                  "detector_threshold"}
    assert want <= fields, want - fields
    nb = {kw["contrast_factor_num_bins"] for _, kw, _ in CONTRAST_CONFIGS if "contrast_factor_num_bins" in kw}
    assert min(nb) <= 640 < max(nb) and 641 in nb and 4096 in nb  # both sides of the march / stream contrast kernels' limit


REFUSED = [
    (dict(descriptor_pattern_size=9), -6),
    (dict(descriptor_pattern_size=11), -6),
    (dict(contrast_factor_num_bins=0), -1),
    (dict(contrast_factor_num_bins=4097), -1),
    (dict(base_scale_offset=0.0), -1),
    (dict(base_scale_offset=-1.0), -1),
    (dict(base_scale_offset=float("nan")), -1),
    (dict(base_scale_offset=6.0001), -1),
    (dict(derivative_factor=0.2), -6),                         # detector sigma 0 at level 0 (round(1.6 * 0.2))
    (dict(derivative_factor=2.5), -6),                         # detector sigma 7 at sublevel 3 (round(2.69 * 2.5))
    (dict(num_sublevels=64, max_octave_evolution=1), -6),      # a one-step FED schedule (fed_tau.rs:95 never ends)
    (dict(num_sublevels=65, max_octave_evolution=1), -1),      # more than 64 levels
    (dict(num_sublevels=13, max_octave_evolution=5), -1),
    (dict(num_sublevels=0), -1),
    (dict(max_octave_evolution=0), -1),
    (dict(descriptor_channels=0), -1),
    (dict(descriptor_channels=4), -1),
]


@pytest.mark.parametrize("kw,status", REFUSED, ids=[",".join(f"{k}={v}" for k, v in r[0].items()) for r in REFUSED])
def test_refused_configs(amd, kw, status):
    with pytest.raises(amd.AkazeError) as e:
        amd.plan_levels(FRAME_W, FRAME_H, amd.Config(**kw))
    assert e.value.status == status, str(e.value)


@pytest.mark.parametrize("kw", [dict(base_scale_offset=6.0, derivative_factor=0.25), dict(contrast_factor_num_bins=4096),
                                dict(contrast_factor_num_bins=1), dict(contrast_percentile=float("inf")),
                                dict(contrast_percentile=float("nan")), dict(contrast_percentile=-0.5),
                                dict(num_sublevels=10, max_octave_evolution=6), dict(derivative_factor=0.32), dict(derivative_factor=2.4)])
def test_accepted_edges(amd, kw):
    """The edges that are accepted: ceil(base_scale_offset) == 6, 1 and 4096 bins, any percentile, 60 planned levels (40 fit the frame), detector sigma 1 and 6 at the ends of derivative_factor."""
    assert len(amd.plan_levels(FRAME_W, FRAME_H, amd.Config(**kw))) > 0


def sweep_images(ref, shape=(96, 130)):
    """The op tests' inputs: a random frame, power-of-two-scaled copies of one tile with flat gaps wider than every stencil
    halo (gradient magnitudes exact 2^-k multiples of the maximum: they fall on bin edges), the same built from u8 values
    (2x/255 == 2 (x/255) in f32), and a random u8 frame."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    out = [rng.random(shape, dtype=np.float32)]
    tile = rng.random((20, 20), dtype=np.float32)
    tile_u8 = rng.integers(0, 32, (20, 20))
    copies = (lambda k: tile * np.float32(2.0 ** -k), lambda k: u8_unit(tile_u8 << k))
    for copy in copies:
        img = np.zeros(shape, np.float32)
        k = 0
        for y in range(12, h - 31, 32):  # gaps of 12 flat pixels: wider than the 7-tap blur and the Scharr together
            for x in range(12, w - 31, 32):
                img[y:y + 20, x:x + 20] = copy(k % 4)
                k += 1
        assert k >= 4
        out.append(img)
    out.append(u8_unit(rng.integers(0, 256, shape)))
    return np.stack(out)


def u8_unit(a):
    """u8 -> f32 in [0, 1] as image.rs:136 converts it"""
    return (np.asarray(a).astype(np.uint8).astype(np.float32) * np.float32(1.0)) / np.float32(255.0)


PERCENTILE_EXTRAS = [-0.5, float("nan"), 0.0, 1e-9, 0.7, 1.0, 1.5, 1e300, float("inf")]


@pytest.mark.parametrize("nbins", [1, 2, 7, 300, 641, 4096])
@pytest.mark.parametrize("gscale", [0.5, 1.0, 2.5])
def test_numpy_contrast_factor_is_the_oracles(ref, nbins, gscale):
    """The float64 restatement above against the oracle's compute_contrast_factor, on the op tests' inputs, at the extra
    percentiles (the saturating threshold included) and at percentiles either side of several bin edges."""
    imgs = sweep_images(ref)
    for img in imgs:
        blurred = ref.gaussian_blur(img, gscale)
        hist = gradient_histogram(ref.scharr(blurred, True, False, 1), ref.scharr(blurred, False, True, 1), nbins)
        ps = list(PERCENTILE_EXTRAS)
        for t in edge_thresholds(hist[1], 12):
            ps.append(percentile_for(hist[2], t))
        for p in ps:
            assert contrast_from_histogram(*hist, p) == ref.contrast_factor(img, p, gscale, nbins), (nbins, gscale, p)
    flat = np.full((40, 50), 0.25, np.float32)
    for p in PERCENTILE_EXTRAS:
        assert contrast_np(ref, flat, p, gscale, nbins) == ref.contrast_factor(flat, p, gscale, nbins) == 0.0


def edge_thresholds(hist, limit=None, seed=0):
    """Thresholds C - 1, C and C + 1 for the cumulative count C at the end of each bin (a sample of `limit` bins if given):
    a walk to C stops at that bin, a walk to C + 1 goes on, so together they pin every cumulative count."""
    cum = np.cumsum(hist)
    idx = np.arange(len(hist))
    if limit is not None and len(idx) > limit:
        rng = np.random.default_rng(seed)
        idx = np.unique(np.concatenate([idx[:2], idx[-2:], rng.choice(idx, limit, replace=False)]))
    ts = set()
    for j in idx:
        c = int(cum[j])
        ts.update(t for t in (c - 1, c, c + 1) if t >= 1)
    return sorted(ts)


def percentile_for(num_points, t):
    """A percentile p with int(num_points * p) == t (checked)."""
    if num_points == 0:
        return float(t)
    p = t / num_points
    while sat_usize(num_points * p) < t:
        p = float(np.nextafter(p, np.inf))
    while sat_usize(num_points * p) > t:
        p = float(np.nextafter(p, -np.inf))
    assert sat_usize(num_points * p) == t
    return p


@pytest.mark.parametrize("kw", [{}, dict(contrast_factor_num_bins=4096, contrast_percentile=0.93), dict(contrast_percentile=math.inf)])
def test_numpy_contrast_factor_of_an_extraction(amd, ref, kw):
    """The extraction's contrast factor is compute_contrast_factor(Lt0, percentile, 1.0, nbins) with Lt0 the level-0 blur
    (lib.rs:56-69): the restatement on the oracle's Lt0 gives the oracle's extraction its value."""
    cfg = amd.Config(**kw)
    frame = amd.synth_frame(320, 240, 500)
    rf = ref.extract(frame, ref.default_config(**kw))
    lt0 = ref.gaussian_blur(u8_unit(frame), 1.6)
    assert np.array_equal(lt0, rf.plane(0, "Lt"))
    assert contrast_np(ref, lt0, cfg.contrast_percentile, 1.0, cfg.contrast_factor_num_bins) == rf.contrast
    rf.close()
