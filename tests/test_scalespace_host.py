"""The front half of AKAZE, from the frame to Ldet, on the CPU: the numpy statement (tests/scalespace_numpy.py, written from
the reference's text) against the oracle -- every single op, the contrast factor, the FED schedule, and whole pyramids for
every case of tests/scalespace_cases.py -- so that the float planes have a second, independent witness; the cases are shown to
have teeth (every mutation switch of the statement changes a plane or the contrast factor of the cases CATCHES names, every
case changes under some switch); the two quirks of the reference's flat filter loops are shown to be invisible; and the chain
pyramid -> extrema_numpy.detect -> mldb_numpy.describe gives the oracle's keypoints and descriptor bytes.  Everything is
compared for equality; no GPU call."""
import numpy as np
import pytest

import scalespace_cases as X
import scalespace_numpy as S
from test_gpu_ops import FED_TAUS

OP_SHAPES = [(3, 3), (5, 64), (64, 5), (37, 53), (101, 259)]  # (h, w)
CHAIN_FRAMES = [(322, 200, 21, 3), (322, 200, 16, 1), (517, 389, 2, 3), (517, 389, 6, 1)]  # (w, h, synthetic frame, channels)
KP_FIELDS = ("x", "y", "response", "size", "octave", "class_id", "angle")

# per switch, the cases that MUST differ under it; test_teeth prints the whole matrix
CATCHES = {
    "half_row_major": ("160x80", "163x81", "322x200"),           # a second octave
    "pm_g2_f32": ("163x81", "322x200", "noise"),
    "tau_f64": ("163x81", "130x66", "noise"),
    "fed_sum_order": ("163x81", "130x66", "noise"),
    "fed_border_zero_terms": ("pct0",),                           # zero conductivity: fluxes are signed zeros (as words)
    "contrast_whole_image": ("12x40", "2000x24"),                 # strips: a sixth of the pixels lie on the border
    "contrast_zero_counted": ("blocky",),                         # flat blocks: interior pixels without a gradient
    "contrast_no_clamp_guard": ("pct1",),                         # the threshold is every point: one point short, 0.03
    "contrast_thr_le": ("pct0",),                                 # threshold 0: `<=` starts the walk
    "k_not_scaled_per_octave": ("160x80", "163x81", "322x200"),
    "lt_from_level0": ("11x11", "163x81", "322x200"),
    "lsmooth0_blurred": ("11x11", "163x81"),
    "scharr_vertical_pass_first": ("11x11", "12x40", "163x81"),
    "taps_reversed": ("163x81", "base2.5"),
    "lxy_from_ly": ("11x11", "163x81", "deriv2.3"),
    "lx_ly_of_flow_kept": ("11x11", "163x81", "2000x24"),
    "sigma_round_half_even": ("half_sigma",),
    "ldet_quat_last_f64": ("163x81", "322x200"),
    "blur_size_round": ("base1.3",),
}


def rand_img(h, w, seed, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (h, w)).astype(np.float32)


def same(a, b, what=None):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert not np.isnan(a).any() and not np.isnan(b).any(), what
    assert np.array_equal(a, b), (what, int((a != b).sum()), np.argwhere(a != b)[:3].tolist())


stated = X.stated


def differs(name, mut):
    how = X.case(name)[3]
    (la, ka), (lb, kb) = stated(name), stated(name, mut)
    if not X.contrast_equal(ka, kb):
        return True
    return any(not X.planes_equal(a["planes"][p], b["planes"][p], how) for a, b in zip(la, lb) for p in S.PLANES)


# ---- single ops against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OP_SHAPES)
def test_filters(ref, shape):
    h, w = shape
    for klen in (3, 5, 7, 9, 11, 13):
        if not S.filter_fits(w, h, klen):
            continue
        img = rand_img(h, w, klen, -1.0)
        kern = np.random.default_rng(klen + 1).standard_normal(klen).astype(np.float32)
        same(S.horizontal_filter(img, kern), ref.horizontal_filter(img, kern), ("horizontal", klen))
        same(S.vertical_filter(img, kern), ref.vertical_filter(img, kern), ("vertical", klen))


@pytest.mark.parametrize("shape", OP_SHAPES)
def test_gaussian_blur_half_size_scharr(ref, shape):
    h, w = shape
    img = rand_img(h, w, 2, -1.0)
    for sigma in (0.7, 1.0, 1.3, 1.6, 2.5, 4.0, 5.5):
        n = S.gaussian_kernel_size(sigma)
        assert np.array_equal(S.gaussian_kernel(np.float32(sigma), n), ref.gaussian_kernel(sigma, n)), sigma
        if S.filter_fits(w, h, n):
            same(S.gaussian_blur(img, sigma), ref.gaussian_blur(img, sigma), ("blur", sigma))
    same(S.half_size(img), ref.half_size(img), "half_size")
    for sigma in range(1, 7):
        m, o = S.scharr_kernels(sigma)
        rm, ro = ref.scharr_kernels(sigma)
        assert np.array_equal(m, rm) and np.array_equal(o, ro), sigma
        if not S.filter_fits(w, h, 2 * sigma + 1):
            continue
        for xo, yo in ((True, False), (False, True), (True, True), (False, False)):
            same(S.scharr(img, xo, yo, sigma), ref.scharr(img, xo, yo, sigma), ("scharr", xo, yo, sigma))


@pytest.mark.parametrize("shape", OP_SHAPES)
def test_pm_g2_fed_contrast(ref, shape):
    h, w = shape
    lx, ly = rand_img(h, w, 5, -0.2, 0.2), rand_img(h, w, 6, -0.2, 0.2)
    for k in (0.0043, 0.03, 0.5, (0.0123 * 0.75) * 0.75):
        same(S.pm_g2(lx, ly, k), ref.pm_g2(lx, ly, k), ("pm_g2", k))
    lt0, c = rand_img(h, w, 9), rand_img(h, w, 10)
    lt, rlt = lt0, lt0
    for n, tau in enumerate(FED_TAUS):  # 1 .. 13 steps: every prefix is compared
        lt, step = S.calculate_step(lt, c, tau)
        rlt, rstep = ref.fed_step(rlt, c, tau)
        same(lt, rlt, ("Lt", n + 1))
        same(step, rstep, ("Lstep", n + 1))
    for img in (lt0, lx, rand_img(h, w, 8, 0.0, 255.0)):
        for pct, nbins in ((0.7, 300), (1.0, 300), (0.0, 300), (0.7, 1), (0.5, 641), (0.93, 4096), (float("inf"), 7), (float("nan"), 7)):
            got, want = S.compute_contrast_factor(img, pct, 1.0, nbins), ref.contrast_factor(img, pct, 1.0, nbins)
            assert got == want, (pct, nbins, got, want)
    flat = np.full((h, w), 0.25, np.float32)
    assert S.compute_contrast_factor(flat, 0.7, 1.0, 300) == ref.contrast_factor(flat, 0.7, 1.0, 300) == 0.0


def config_space(amd):
    """the Configs tests/test_config_space.py and tests/test_gpu_config.py run or accept at their edges"""
    from test_gpu_config import CONFIGS, CONTRAST_CONFIGS
    kws = [kw for _, kw, _ in CONFIGS + CONTRAST_CONFIGS] + [
        {}, dict(base_scale_offset=6.0, derivative_factor=0.25), dict(num_sublevels=10, max_octave_evolution=6),
        dict(derivative_factor=0.32), dict(derivative_factor=2.4), dict(num_sublevels=5, max_octave_evolution=5)]
    return kws + list(X.CONFIGS.values())


def test_fed_tau_and_level_plan_over_the_config_space(amd, ref):
    """every process time the accepted Config space reaches: the tau bytes against the oracle's fed_tau, and the whole level
    plan (etime, esigma, octave, sublevel, sigma_size, sizes, the detector's sigma, tau) against the library's planner"""
    from test_gpu_config import FRAME_H, FRAME_W
    times = set()
    for kw in config_space(amd):
        plan = S.allocate_evolutions(FRAME_W, FRAME_H, X.config(**kw))
        lib_plan = amd.plan_levels(FRAME_W, FRAME_H, amd.Config(**kw))
        assert len(plan) == len(lib_plan), kw
        for i, (a, b) in enumerate(zip(plan, lib_plan)):
            for f in ("etime", "esigma", "octave", "sublevel", "sigma_size"):
                assert a[f] == b[f], (kw, i, f)
            assert a["tau"].tobytes() == b["tau"].tobytes(), (kw, i)
            assert S.detector_sigma(a["esigma"], a["octave"], X.config(**kw).derivative_factor) == b["det_sigma"], (kw, i)
            if i:
                times.add(a["etime"] - plan[i - 1]["etime"])
    assert len(times) > 100
    for t in sorted(times):
        assert S.fed_tau_by_process_time(t).tobytes() == ref.fed_tau(t).tobytes(), t
        assert S.fed_tau_by_process_time(t, 1, 0.25, False).tobytes() == ref.fed_tau(t, 1, 0.25, False).tobytes(), t
    with pytest.raises(ValueError):
        S.fed_tau_by_process_time(0.1)  # one step: the reference's reordering never ends; the oracle refuses it too
    with pytest.raises(ValueError):
        ref.fed_tau(0.1)


def test_half_sigma_config_lies_on_a_half(amd):
    """The accepted Config space does hold a detector sigma exactly on .5 (scalespace_cases.HALF_SIGMA), so
    sigma_round_half_even stays a switch; and base_scale_offset=2.5 and derivative_factor=2.3 are two configs here: together
    they put detector sigma 7 on sublevel 1, which the library refuses."""
    cfg = X.config(**X.HALF_SIGMA)
    lv0 = S.allocate_evolutions(*X.CONFIG_SIZE, cfg)[0]
    v = lv0["esigma"] * cfg.derivative_factor / 2.0 ** float(lv0["octave"])
    assert v == 2.5 and S.detector_sigma(lv0["esigma"], 0, cfg.derivative_factor) == 3
    assert S.detector_sigma(lv0["esigma"], 0, cfg.derivative_factor, ("sigma_round_half_even",)) == 2
    assert amd.plan_levels(*X.CONFIG_SIZE, amd.Config(**X.HALF_SIGMA))[0]["det_sigma"] == 3
    with pytest.raises(amd.AkazeError) as e:
        amd.plan_levels(*X.CONFIG_SIZE, amd.Config(base_scale_offset=2.5, derivative_factor=2.3))
    assert e.value.status == -6
    for kw in X.CONFIGS.values():
        assert len(amd.plan_levels(*X.CONFIG_SIZE, amd.Config(**kw))) == 2 * X.config(**kw).num_sublevels


# ---- whole pyramids against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_pyramid_against_oracle(ref, name):
    _, frame, kw, how = X.case(name)
    levels, contrast = stated(name)
    rf = ref.extract(frame, ref.default_config(**kw))
    assert rf.num_levels == len(levels)
    assert X.contrast_equal(contrast, rf.contrast), (contrast, rf.contrast)
    for l, lv in enumerate(levels):
        info = rf.level_info(l)
        for f in ("etime", "esigma", "octave", "sublevel", "sigma_size", "w", "h"):
            assert info[f] == lv[f], (l, f, info[f], lv[f])
        assert info["tau"].tobytes() == lv["tau"].tobytes(), l
        for p in S.PLANES:
            a, b = lv["planes"][p], rf.plane(l, p)
            assert a.shape == b.shape, (l, p, a.shape, b.shape)
            assert X.planes_equal(a, b, how), (l, p, int((a != b).sum()))
    if name in ("flat", "pct0"):
        assert contrast == 0.0 and np.isnan(levels[-1]["planes"]["Lt"]).all() == (name == "flat")
    rf.close()


def test_cases_are_what_they_say():
    """the regimes the scaled frames are there for, on the statement's own planes"""
    from range_cases import subnormal_share, zero_share
    cat = lambda name, p: np.concatenate([l["planes"][p].ravel() for l in stated(name)[0] if l["planes"][p].size])
    d = cat("ldet_underflow", "Ldet")
    assert zero_share(d) >= 0.05 and subnormal_share(d) >= 0.05
    assert subnormal_share(cat("deriv_subnormal", "Lx")) > 0.5 and subnormal_share(cat("deriv_subnormal", "Lstep")) > 0.5
    assert not cat("deriv_subnormal", "Ldet").any()
    assert [len(stated(n)[0]) for n in ("159x79", "160x80", "322x200")] == [4, 8, 12]
    # a contrast factor of 0 makes the conductivity 0 wherever there is a gradient: fluxes that are zeros of either sign
    assert any((l["planes"]["Lstep"].view(np.uint32) == 0x80000000).any() for l in stated("pct0")[0][1:])
    assert not any((l["planes"]["Lflow"] == 0).any() for l in stated("blocky")[0][1:])
    assert len(S.gaussian_kernel(np.float32(2.5), S.gaussian_kernel_size(2.5))) == 7
    sig = lambda name: {S.detector_sigma(l["esigma"], l["octave"], X.config(**X.case(name)[2]).derivative_factor) for l in stated(name)[0]}
    assert sig("base2.5") == sig("deriv2.3") == {4, 5, 6} and sig("163x81") == {2, 3, 4}


# ---- teeth ----------------------------------------------------------------------------------------------------------------
def test_teeth():
    """Every switch changes a plane or the contrast factor of the cases CATCHES names for it, no switch is left uncaught, and
    no case is decoration: each one changes under at least one switch.  Statement against statement: the code under test has
    no say."""
    matrix = {s: [n for n in X.CASE_NAMES if differs(n, (s,))] for s in S.SWITCHES}
    for s in S.SWITCHES:
        print(f"{s:27s} caught by {matrix[s]}")
    assert set(CATCHES) == set(S.SWITCHES)
    for s, must in CATCHES.items():
        for n in must:
            assert n in X.CASE_NAMES and n in matrix[s], (s, n)
        assert matrix[s], s
    # fed_border_zero_terms moves the sign of zeros only: no case that is compared by value may see it
    assert all(X.case(n)[3] == "words" for n in matrix["fed_border_zero_terms"])
    caught = {n for v in matrix.values() for n in v}
    for n in X.CASE_NAMES:
        assert n in caught, n


# ---- the quirks of the flat filter loops ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OP_SHAPES + [(11, 11), (24, 2000)])
def test_row_wrap_and_unprocessed_pixel_are_invisible(shape):
    """image.rs:286 / :323 stop one pixel short of the range the taps cover, and the horizontal loop runs across row ends, so
    that the first and last hw pixels of a row hold sums over two rows.  fill_border (:239-260) overwrites every such pixel: with
    the loops run to the end, or with the wrapped sums zeroed, every output is the same WORDS.  A statement about the reference:
    whoever "fixes" either in one implementation changes nothing, and need not."""
    h, w = shape
    for klen in (3, 5, 7, 9, 11, 13):
        if not S.filter_fits(w, h, klen):
            continue
        img = rand_img(h, w, 40 + klen, -1.0)
        kern = np.random.default_rng(klen).standard_normal(klen).astype(np.float32)
        for fn in (S.horizontal_filter, S.vertical_filter):
            want = fn(img, kern).view(np.uint32)
            for mut in (("filter_full_range",), ("filter_no_wrap",), S.INVISIBLE):
                assert np.array_equal(fn(img, kern, mut).view(np.uint32), want), (fn.__name__, klen, mut)
    # and they are real: before fill_border the outputs do differ
    img, kern = rand_img(9, 9, 1, -1.0), np.float32([1, 2, 3])
    flat = np.zeros(81, np.float32)
    for k in (-1, 0, 1):
        flat[1:79] += kern[k + 1] * img.ravel()[1 + k:79 + k]
    assert flat[9] != 0 and flat[17] != 0 and flat[79] == 0  # wrapped sums at a row's ends; the last but one pixel untouched


# ---- the chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,idx,ch", CHAIN_FRAMES)
def test_chain_gives_the_oracles_keypoints_and_descriptors(amd, ref, w, h, idx, ch):
    """pyramid() -> extrema_numpy.detect on its Ldet -> mldb_numpy.describe on its Lt, Lx, Ly: a numpy AKAZE from the frame to
    the descriptor bytes that shares no code with the oracle, equal to ref.extract in every keypoint field (the angle's bits
    too) and every descriptor byte."""
    frame = amd.synth_frame(w, h, idx)
    kps, desc, _, contrast = S.extract(frame, X.config(descriptor_channels=ch))
    rf = ref.extract(frame, ref.default_config(descriptor_channels=ch))
    rk = rf.keypoints()
    print(f"{w}x{h} frame {idx}, {ch} channels: {len(kps)} keypoints")
    assert len(kps) == len(rk) >= 15 and contrast == rf.contrast
    for f in KP_FIELDS:
        a, b = np.ascontiguousarray(kps[f]), np.ascontiguousarray(rk[f])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), f
    assert np.array_equal(desc, rf.descriptors())
    rf.close()
