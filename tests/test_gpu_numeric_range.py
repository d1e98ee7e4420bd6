"""Every plane kernel and the whole extraction against the oracle over the f32 range: inputs scaled by powers of two from
2^-149 (the last bit of the format) to 2^62 (the largest unit-range content whose pyramid stays finite), so that the planes
are subnormal, part subnormal and part zero, or huge -- tests/range_cases.py, whose premises tests/test_numeric_range_host.py
holds on the oracle alone.  A kernel that flushes subnormals, a reciprocal shortcut, or a float-to-key mapping that collapses
subnormals fails here.  Bar: bit-exact, compared by value, no tolerance."""
import functools

import numpy as np
import pytest

import range_cases as R
from test_gpu_extract import assert_same_result
from test_gpu_ops import dev, host, same

pytestmark = pytest.mark.gpu

ALL_SHAPES = R.OP_SHAPES + [R.STRIP_SHAPE]


@pytest.fixture(scope="module", autouse=True)
def drop_cached_oracle_results():
    """the shared oracle results are freed with the module, not at interpreter exit"""
    yield
    R.oracle_result.cache_clear()


def exps_of(op):
    return R.COMMON_EXPS + R.CROSSING[op]


def check_crossing(op, e, *outputs):
    """at the exponents where the op's output crosses the subnormal boundary, the oracle's output really is subnormal"""
    if e in R.CROSSING[op]:
        for out in outputs:
            assert R.subnormal_share(out) > 0.25, (op, e, R.subnormal_share(out))


# ---- per op --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("klen", [5, 9, 13])
def test_horizontal_vertical_filter(ctx, ref, klen):
    kern = np.random.default_rng(klen + 1).standard_normal(klen).astype(np.float32)
    for shape in R.OP_SHAPES:
        for e in exps_of("filter"):
            img = R.op_plane(shape, 1, e)
            eh, ev = ref.horizontal_filter(img, kern), ref.vertical_filter(img, kern)
            if klen == 9:
                check_crossing("filter", e, eh, ev)
            same(host(ctx.horizontal_filter(dev(img), kern)), eh)
            same(host(ctx.vertical_filter(dev(img), kern)), ev)


@functools.lru_cache(maxsize=None)
def blur_expected(ref, shape, e, sigma):
    return ref.gaussian_blur(R.op_plane(shape, 2, e), sigma)


@pytest.mark.parametrize("mode", [0, 1, 3], ids=["tiled", "stream", "march"])
@pytest.mark.parametrize("sigma", [1.0, 1.6, 2.5])
def test_gaussian_blur(ctx, ref, sigma, mode):
    ctx.set_prep_mode(mode)
    try:
        for shape in ALL_SHAPES:
            for e in exps_of("gaussian_blur"):
                exp = blur_expected(ref, shape, e, sigma)
                check_crossing("gaussian_blur", e, exp)
                same(host(ctx.gaussian_blur(dev(R.op_plane(shape, 2, e)), sigma)), exp)
    finally:
        ctx.set_prep_mode(2)


def test_half_size(ctx, ref):
    for shape in ALL_SHAPES:
        for e in exps_of("half_size"):
            img = R.op_plane(shape, 3, e)
            exp = ref.half_size(img)
            check_crossing("half_size", e, exp)
            same(host(ctx.half_size(dev(img))), exp)


@pytest.mark.parametrize("sigma", [1, 2, 3, 4, 5, 6])
def test_scharr(ctx, ref, sigma):
    for shape in R.OP_SHAPES:
        for e in exps_of("scharr"):
            img = R.op_plane(shape, 4, e)
            ex, ey = ref.scharr(img, True, False, sigma), ref.scharr(img, False, True, sigma)
            check_crossing("scharr", e, ex, ey)
            same(host(ctx.scharr(dev(img), True, False, sigma)), ex)
            same(host(ctx.scharr(dev(img), False, True, sigma)), ey)


@functools.lru_cache(maxsize=None)
def detector_expected(ref, shape, e, sigma):
    return R.detector_expected(ref, R.op_plane(shape, 60 + sigma, e), sigma)


@pytest.mark.parametrize("mode", [0, 4, 5, 2], ids=["multi_kernel", "tiled", "march", "auto"])
@pytest.mark.parametrize("sigma", [1, 2, 3, 4, 5, 6])
def test_detector_response(ctx, ref, sigma, mode):
    """a batch of two planes at different exponents (every exponent in either place), with and without the second
    derivatives kept; Ldet lies 2e below its input, so it crosses the subnormal boundary near e = -61"""
    exps = exps_of("detector_response")
    ctx.set_detector_mode(mode)
    try:
        for shape in ALL_SHAPES:
            for i, e0 in enumerate(exps):
                pair = (e0, exps[(i + 1) % len(exps)])
                ls = np.stack([R.op_plane(shape, 60 + sigma, e) for e in pair])
                full = {k: host(v) for k, v in ctx.detector_response(dev(ls), sigma).items()}
                lean = {k: host(v) for k, v in ctx.detector_response(dev(ls), sigma, keep_second=False).items()}
                assert set(lean) == {"Lx", "Ly", "Ldet"}
                for j, e in enumerate(pair):
                    exp = detector_expected(ref, shape, e, sigma)
                    check_crossing("detector_response", e, exp["Ldet"])
                    for name, v in exp.items():
                        same(full[name][j], v)
                    for name in ("Lx", "Ly", "Ldet"):
                        same(lean[name][j], exp[name])
    finally:
        ctx.set_detector_mode(2)


def _k_of(e):
    return 0.0123 * 2.0 ** (-149 if e == "bits" else e)


def test_pm_g2_and_flow(ctx, ref):
    """k follows the planes (k = 0.0123 * 2^e, an f64), so the conductivity stays in (0, 1]; then unit-range planes with a k
    63 and 70 binades below them, where the conductivity itself is subnormal and pm_g2's quotient leaves the range of its
    refined reciprocal (csrc/akz_pm_g2.hpp: x >= 2^64 takes the division)"""
    cases = [(e, e, False) for e in R.COMMON_EXPS] + [(0, ek, True) for ek in R.CROSSING["pm_g2_k"]] + \
            [(0, ek, False) for ek in R.PM_G2_K_EXTRA]
    for shape in R.OP_SHAPES:
        for e, ek, crossing in cases:
            k = _k_of(ek)
            lx, ly, ls = R.op_plane(shape, 5, e), R.op_plane(shape, 6, e), R.op_plane(shape, 7, e)
            exp = ref.pm_g2(lx, ly, k)
            gx, gy = ref.scharr(ls, True, False, 1), ref.scharr(ls, False, True, 1)
            exp_flow = ref.pm_g2(gx, gy, k)
            if crossing:
                assert R.subnormal_share(exp) > 0.25 and R.subnormal_share(exp_flow) > 0.25
            same(host(ctx.pm_g2(dev(lx), dev(ly), k)), exp)
            same(host(ctx.flow(dev(ls), k)), exp_flow)
            same(host(ctx.flow(dev(ls), k, 2)), ref.pm_g2(gx, gy, (k * 0.75) * 0.75))  # multiplied step by step (lib.rs:84)


@pytest.mark.parametrize("tiny_flow", [False, True], ids=["flow_unit", "flow_2^-130"])
@pytest.mark.parametrize("mode", [2, 0], ids=["k_fed_own", "k_fed_step"])
@pytest.mark.parametrize("shape", R.FED_SHAPES)
def test_fed_steps(ctx, ref, shape, mode, tiny_flow):
    flow = R.fed_flow(shape, 10, tiny_flow)
    ctx.set_fed_mode(mode)
    try:
        for e in exps_of("fed_steps"):
            lt = R.op_plane(shape, 9, e)
            exp, step = R.fed_expected(ref, lt, flow, R.FED_TAUS)
            check_crossing("fed_steps", e, exp)
            d_lt = dev(lt)
            d_step = ctx.fed_steps(d_lt, dev(flow), R.FED_TAUS, want_lstep=True)
            same(host(d_lt), exp)
            same(host(d_step), step)
    finally:
        ctx.set_fed_mode(2)


@functools.lru_cache(maxsize=None)
def contrast_expected(ref, shape, nbins):
    imgs = R.contrast_images(ref, shape, R.CONTRAST_EXPS)
    return imgs, [ref.contrast_factor(img, 0.7, 1.0, nbins) for img in imgs]


@pytest.mark.parametrize("mode", [0, 1, 3], ids=["tiled", "stream", "march"])
@pytest.mark.parametrize("nbins", [300, 641])
def test_contrast_factor(ctx, ref, nbins, mode):
    """blurred noise on both sides of where an f32 squared gradient magnitude would underflow (the reference squares in
    f64): every exponent in one batch, and batches of three whose per-image maxima lie 30 and more orders of magnitude apart"""
    ctx.set_prep_mode(mode)
    try:
        for shape in ALL_SHAPES:
            imgs, want = contrast_expected(ref, shape, nbins)
            got = host(ctx.contrast_factor(dev(imgs), 0.7, 1.0, nbins))
            assert [float(v) for v in got] == want, (shape, got, want)
            for batch in R.CONTRAST_BATCHES:
                idx = [R.CONTRAST_EXPS.index(e) for e in batch]
                got = host(ctx.contrast_factor(dev(imgs[idx]), 0.7, 1.0, nbins))
                assert [float(v) for v in got] == [want[i] for i in idx], (shape, batch, got)
            for i in (1, 4, 7):  # ... and alone
                assert float(host(ctx.contrast_factor(dev(imgs[i]), 0.7, 1.0, nbins))[0]) == want[i], (shape, R.CONTRAST_EXPS[i])
    finally:
        ctx.set_prep_mode(2)


# ---- the whole extraction ------------------------------------------------------------------------------------------------
def _labelled(label, fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError as err:
        raise AssertionError(f"{label}: {err}") from err


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_extraction_under_every_forced_form(ctx, amd, ref, regime, shape):
    """every side of every gate (tests/test_gpu_gates.py: the marches, streaming, tiled, one launch per FED step, 16-row bands,
    selection and sort on the device and on the host) at detector_threshold = 0: all planes, keypoints and descriptors; then
    the default form once more with a threshold that cuts most keypoints, moved along with Ldet: 1e-4 * 2^2e"""
    import torch
    from test_gpu_gates import FORCED
    f = R.regime_frame(amd, shape, regime)
    rf = R.oracle_result(ref, amd, shape, regime)
    d = torch.from_numpy(f[None]).cuda()
    torch.cuda.synchronize()
    cfg = amd.Config(detector_threshold=0.0)
    try:
        for label, force, undo in FORCED:
            force(ctx)
            try:
                res = ctx.extract_features(d, cfg)
                _labelled(f"{regime} {label}", assert_same_result, res, rf)
                res.close()
                res = ctx.extract_begin(d, cfg).finish()
                _labelled(f"{regime} {label}, begin / finish", assert_same_result, res, rf)
                res.close()
            finally:
                undo(ctx)
    finally:
        for _, _, undo in FORCED:
            undo(ctx)
    thr = float(np.ldexp(1e-4, 2 * R.REGIMES[regime]))
    assert thr > 0.0 and np.isfinite(thr)
    rt = ref.extract(f, ref.default_config(detector_threshold=thr))
    if regime in ("natural", "small_normal", "ldet_subnormal"):
        assert 10 <= rt.num_keypoints < rf.num_keypoints  # the threshold cuts, and not everything
    res = ctx.extract_features(f, amd.Config(detector_threshold=thr))  # (the host f32 entry)
    _labelled(f"{regime} threshold {thr!r}", assert_same_result, res, rt, planes=False)
    res.close()
    rt.close()


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
def test_batch_that_mixes_regimes(ctx, amd, ref, shape):
    """natural, ldet_subnormal and largest_finite frames in one job, through the synchronous call and begin / finish: the
    per-image contrast factor and the per-image candidate lists must not leak across images"""
    import torch
    regimes = ("natural", "ldet_subnormal", "largest_finite")
    frames = np.stack([R.regime_frame(amd, shape, r) for r in regimes])
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    cfg = amd.Config(detector_threshold=0.0)
    sync = ctx.extract_features(d, cfg)
    asyn = ctx.extract_begin(d, cfg).finish()
    from_host = ctx.extract_begin_host(frames, cfg).finish()  # (akz_extract_begin_host_f32: the upload is the job's own)
    for i, r in enumerate(regimes):
        rf = R.oracle_result(ref, amd, shape, r)
        _labelled(f"image {i} ({r}), synchronous call", assert_same_result, sync, rf, img=i)
        _labelled(f"image {i} ({r}), begin / finish", assert_same_result, asyn, rf, img=i)
        _labelled(f"image {i} ({r}), begin / finish from host memory", assert_same_result, from_host, rf, img=i)
    for res in (sync, asyn, from_host):
        res.close()


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
@pytest.mark.parametrize("regime", ["ldet_subnormal", "deriv_subnormal", "last_bits", "largest_finite"])
def test_lean_result_recomputes_its_planes_on_fetch(ctx, amd, ref, regime, shape):
    """without AKZ_KEEP_ALL_PLANES the second derivatives and Lstep are not kept: fetching them runs the per-level kernels
    again, on subnormal and on huge planes, one plane at a time and as the whole pyramid in one call"""
    rf = R.oracle_result(ref, amd, shape, regime)
    res = ctx.extract_features(R.regime_frame(amd, shape, regime), amd.Config(detector_threshold=0.0), keep_all_planes=False)
    _labelled(f"{regime}, plane by plane", assert_same_result, res, rf)
    for lvl, planes in enumerate(res.pyramid()):
        for name, a in planes.items():
            b = rf.plane(lvl, name)
            assert a.shape == b.shape, (lvl, name)
            if a.size:
                _labelled(f"{regime}, whole pyramid, level {lvl} {name}", same, a, b)
    res.close()


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
@pytest.mark.parametrize("regime", ["natural", "ldet_subnormal"])
def test_signed_frame(ctx, amd, ref, regime, shape):
    """content minus 0.5: Lt of both signs"""
    f = R.regime_frame(amd, shape, regime, signed=True)
    assert (f < 0).mean() > 0.2 and (f > 0).mean() > 0.2
    rf = R.oracle_result(ref, amd, shape, regime, True)
    assert rf.num_keypoints >= 10
    res = ctx.extract_features(f, amd.Config(detector_threshold=0.0))
    assert_same_result(res, rf)
    res.close()


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
def test_planes_and_contrast_scale_with_the_frame_without_the_oracle(ctx, amd, shape):
    """The GPU's own planes and contrast factor at small_normal and large are ldexp of its natural result: by 0 for Lflow, 2e
    for Ldet and e otherwise (what the oracle does: tests/test_numeric_range_host.py).  A failure here and not above, or the
    other way round, tells scale handling from everything else."""
    cfg = amd.Config(detector_threshold=0.0)
    nat = ctx.extract_features(R.regime_frame(amd, shape, "natural"), cfg)
    base = nat.pyramid()
    for regime in ("small_normal", "large"):
        e = R.REGIMES[regime]
        res = ctx.extract_features(R.regime_frame(amd, shape, regime), cfg)
        assert res.contrast() == float(np.ldexp(nat.contrast(), e)), regime
        for lvl, (a, b) in enumerate(zip(base, res.pyramid())):
            for name in R.PLANES:
                assert a[name].shape == b[name].shape
                if a[name].size:
                    _labelled(f"{regime} level {lvl} {name}", same, b[name], np.ldexp(a[name], R.PLANE_EXPONENT[name] * e))
        res.close()
    nat.close()


# the describe test's frames: two regimes, and the exponent at which the SQUARES of the orientation window's sums underflow
# (the oracle gives 265 different angles for the 540 keypoints there, 500 and more at e = -64, one from e = -76 down)
DESCRIBE_EXPS = {"deriv_subnormal": R.REGIMES["deriv_subnormal"], "lt_subnormal": R.REGIMES["lt_subnormal"],
                 "orientation_underflow": -68}


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
@pytest.mark.parametrize("regime", list(DESCRIBE_EXPS))
def test_orientation_and_mldb_on_subnormal_derivatives(ctx, amd, ref, regime, shape):
    """No extrema survive where Lx and Ly are subnormal, so k_orientation and k_mldb get a grid of caller-supplied keypoints
    on that pyramid (as tests/test_gpu_describe.py does), inside the planes, where the oracle's unchecked reads are defined.
    With subnormal derivatives every window's squared length underflows and the oracle returns the same angle throughout;
    at orientation_underflow only part of them do."""
    import mldb_numpy as M
    w, h, idx = shape
    f = R.frame(amd, w, h, idx, DESCRIBE_EXPS[regime])
    cfg = dict(detector_threshold=0.0)
    res, rf = ctx.extract_features(f, amd.Config(**cfg)), ref.extract(f, ref.default_config(**cfg))
    rows = []
    for lvl, lv in enumerate(amd.plan_levels(w, h)):
        r = 2.0 ** lv["octave"]
        for px in np.linspace(16, lv["w"] - 18, 9):
            for py in np.linspace(16, lv["h"] - 18, 5):
                rows.append((np.float32(px) * r, np.float32(py + 0.5) * r, 0.0, 2.0 * r, lv["octave"], lvl, 0.6, 0))
    kps = np.array(rows, M.KEYPOINT_DTYPE)
    for lvl in range(rf.num_levels):  # what the two ops read is what the oracle read
        for name in ("Lt", "Lx", "Ly"):
            same(res.plane(lvl, name), rf.plane(lvl, name))
        if regime != "orientation_underflow":
            assert res.counts(0)[1] == rf.num_keypoints == 0
            assert R.subnormal_share(rf.plane(lvl, "Lx")) > 0.5 and R.subnormal_share(rf.plane(lvl, "Ly")) > 0.5
    for orient in (True, False):
        want_k, want_d = rf.describe(kps, compute_orientation=orient)
        got_k, got_d = res.describe_keypoints(kps, compute_orientation=orient)
        bad_a = np.flatnonzero(got_k["angle"].view(np.uint32) != want_k["angle"].view(np.uint32))
        bad_d = np.flatnonzero((got_d != want_d).any(axis=1))
        angles = len(np.unique(want_k["angle"]))
        print(f"{regime} {w}x{h} orient={orient}: {len(kps)} keypoints, {angles} different angles, {len(bad_a)} angles and "
              f"{len(bad_d)} descriptors differ")
        assert len(bad_a) == 0 and len(bad_d) == 0, (regime, orient, bad_a[:8], bad_d[:8], kps[bad_a[:3]])
        if orient and regime == "orientation_underflow":
            assert 100 < angles < len(kps) - 100
        assert len(np.unique(want_d, axis=0)) > len(kps) // 2  # the comparisons of subnormal means still tell cells apart
    res.close()
    rf.close()
