"""The kernels of the front half -- every plane op of the C ABI and whole extractions with all planes kept -- against the
numpy statement of the reference (tests/scalespace_numpy.py) on the inputs of tests/scalespace_cases.py.  The oracle is not
consulted here: the statement is the second, independent witness of every float plane (Lt ... Ldet), the contrast factor and
the FED schedule.  Whole extractions run under every forced row of tests/test_gpu_gates.FORCED through both entry points, in
a context forced to the marches and the resident octave kernel, and as batches on the batch and the lone path; the statement
chained with tests/extrema_numpy.py and tests/mldb_numpy.py gives the keypoints and descriptor bytes of extract_features.
Every comparison is an equality (by value; as words on the cases whose zeros carry a sign; NaN positions equal)."""
import numpy as np
import pytest

import scalespace_cases as X
import scalespace_numpy as S
from test_gpu_ops import FED_TAUS
from test_scalespace_host import CHAIN_FRAMES, KP_FIELDS

pytestmark = pytest.mark.gpu

OP_SHAPES = [(3, 3), (5, 64), (64, 5), (33, 130), (37, 53), (101, 259)]  # (h, w)
INFO = ("etime", "esigma", "octave", "sublevel", "sigma_size", "w", "h")


# k_octave_resident (akz_resident.hip) evaluates the flux towards a missing neighbour as an exact zero of EITHER sign instead of
# leaving the term out ("only the sign of a zero can differ"), so where it runs -- prep mode 3 -- a zero of Lt /
# Lstep may carry the other sign than nonlinear_diffusion.rs:84-137 gives it.  That shows only where fluxes are signed zeros:
# the case with a contrast factor of 0.  There, on those paths, values and NaN positions are compared; everywhere else words.
RESIDENT_ROW = "march_px / level_march_px: marches wherever supported"
SIGNED_ZERO_FLUXES = ("pct0",)


def how_under(name, how, resident):
    return "nan" if resident and name in SIGNED_ZERO_FLUXES else how


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(a, b, what=None):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert not np.isnan(a).any() and not np.isnan(b).any(), what
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} of {a.size} values differ, first at {bad[0]}: {a[tuple(bad[0])]!r} vs "
                             f"{b[tuple(bad[0])]!r}")


def rand_img(h, w, seed, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (h, w)).astype(np.float32)


def fed_stated(lt, c, taus):
    """[(Lt, Lstep) after 1, 2, ... steps]"""
    out = []
    for tau in taus:
        lt, step = S.calculate_step(lt, c, tau)
        out.append((lt, step))
    return out


def detector_same(got, exp, what, names=("Lx", "Ly", "Lxx", "Lyy", "Lxy", "Ldet")):
    for name in names:
        same(host(got[name]), exp[name], (what, name))


# ---- single ops of the C ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OP_SHAPES)
def test_filters_and_blur(ctx, shape):
    h, w = shape
    for klen in (3, 5, 7, 9, 11, 13):
        if not S.filter_fits(w, h, klen):
            continue
        img = rand_img(h, w, klen, -1.0)
        kern = np.random.default_rng(klen + 1).standard_normal(klen).astype(np.float32)
        same(host(ctx.horizontal_filter(dev(img), kern)), S.horizontal_filter(img, kern), ("horizontal", klen))
        same(host(ctx.vertical_filter(dev(img), kern)), S.vertical_filter(img, kern), ("vertical", klen))
    img = rand_img(h, w, 2)
    u8 = np.random.default_rng(3).integers(0, 256, (h, w), dtype=np.uint8)
    for sigma in (1.0, 1.3, 1.6, 2.5, 5.5):
        if S.filter_fits(w, h, S.gaussian_kernel_size(sigma)):
            same(host(ctx.gaussian_blur(dev(img), sigma)), S.gaussian_blur(img, sigma), ("blur f32", sigma))
            same(host(ctx.gaussian_blur(dev(u8), sigma)), S.gaussian_blur(S.unit_float(u8), sigma), ("blur u8", sigma))


@pytest.mark.parametrize("shape", OP_SHAPES)
def test_half_size_scharr_pm_g2_flow_contrast(ctx, shape):
    h, w = shape
    img = rand_img(h, w, 4, -1.0)
    same(host(ctx.half_size(dev(img))), S.half_size(img), "half_size")
    for sigma in range(1, 7):
        if not S.filter_fits(w, h, 2 * sigma + 1):
            continue
        for xo, yo in ((True, False), (False, True), (True, True), (False, False)):
            same(host(ctx.scharr(dev(img), xo, yo, sigma)), S.scharr(img, xo, yo, sigma), ("scharr", xo, yo, sigma))
    lx, ly = rand_img(h, w, 5, -0.2, 0.2), rand_img(h, w, 6, -0.2, 0.2)
    for k in (0.0043, 0.03, 0.5):
        same(host(ctx.pm_g2(dev(lx), dev(ly), k)), S.pm_g2(lx, ly, k), ("pm_g2", k))
    ls = rand_img(h, w, 7)
    gx, gy = S.scharr(ls, True, False, 1), S.scharr(ls, False, True, 1)
    k = 0.0123
    same(host(ctx.flow(dev(ls), k)), S.pm_g2(gx, gy, k), "flow")
    same(host(ctx.flow(dev(ls), k, 2)), S.pm_g2(gx, gy, (k * 0.75) * 0.75), "flow, octave 2")  # lib.rs:84, one octave at a time
    if min(w, h) >= 5:  # (the library's lower bound for the contrast factor)
        for src in (ls, S.gaussian_blur(ls, 1.6), rand_img(h, w, 8, 0.0, 255.0)):
            for pct, nbins in ((0.7, 300), (1.0, 300), (0.0, 300), (0.7, 1), (0.5, 641), (0.93, 4096)):
                got = float(host(ctx.contrast_factor(dev(src), pct, 1.0, nbins))[0])
                assert got == S.compute_contrast_factor(src, pct, 1.0, nbins), (pct, nbins)


@pytest.mark.parametrize("mode", [2, 0])  # 2: k_fed_own, 0: one launch per step
@pytest.mark.parametrize("shape", OP_SHAPES)
def test_fed_steps(ctx, shape, mode):
    h, w = shape
    lt, c = rand_img(h, w, 9), rand_img(h, w, 10)
    want = fed_stated(lt, c, FED_TAUS)
    ctx.set_fed_mode(mode)
    try:
        for ntau in (1, 2, 4, 5, 8, 13):
            d_lt = dev(lt)
            d_step = ctx.fed_steps(d_lt, dev(c), FED_TAUS[:ntau], want_lstep=True)
            same(host(d_lt), want[ntau - 1][0], ("Lt", ntau))
            same(host(d_step), want[ntau - 1][1], ("Lstep", ntau))
    finally:
        ctx.set_fed_mode(2)


@pytest.mark.parametrize("mode", [0, 4, 5, 2], ids=["multi_kernel", "tiled", "march", "auto"])
@pytest.mark.parametrize("shape", OP_SHAPES)
def test_detector_response(ctx, shape, mode):
    h, w = shape
    ls = rand_img(h, w, 11, -1.0)
    ctx.set_detector_mode(mode)
    try:
        for sigma in range(1, 7):
            if not S.filter_fits(w, h, 2 * sigma + 1):
                continue
            exp = S.detector_response(ls, sigma)
            detector_same(ctx.detector_response(dev(ls), sigma), exp, sigma)
            lean = ctx.detector_response(dev(ls), sigma, keep_second=False)
            assert set(lean) == {"Lx", "Ly", "Ldet"}
            detector_same(lean, exp, (sigma, "lean"), ("Lx", "Ly", "Ldet"))
    finally:
        ctx.set_detector_mode(2)


def test_batch_of_three_planes_of_unaligned_width(ctx):
    """three planes in one call, 53 columns: no row starts on a 16-byte boundary"""
    h, w = 37, 53
    imgs = np.stack([rand_img(h, w, 20 + s, -1.0) for s in range(3)])
    flows = np.stack([rand_img(h, w, 30 + s) for s in range(3)])
    blur, half = host(ctx.gaussian_blur(dev(imgs), 1.6)), host(ctx.half_size(dev(imgs)))
    sch = host(ctx.scharr(dev(imgs), False, True, 3))
    flow = host(ctx.flow(dev(imgs), 0.0123, 1))
    contrast = host(ctx.contrast_factor(dev(imgs), 0.7, 1.0, 300))
    d_lt = dev(imgs)
    step = host(ctx.fed_steps(d_lt, dev(flows), FED_TAUS[:7], want_lstep=True))
    lt = host(d_lt)
    det = ctx.detector_response(dev(imgs), 2)
    for i in range(3):
        same(blur[i], S.gaussian_blur(imgs[i], 1.6), ("blur", i))
        same(half[i], S.half_size(imgs[i]), ("half_size", i))
        same(sch[i], S.scharr(imgs[i], False, True, 3), ("scharr", i))
        same(flow[i], S.pm_g2(S.scharr(imgs[i], True, False, 1), S.scharr(imgs[i], False, True, 1), 0.0123 * 0.75), ("flow", i))
        assert float(contrast[i]) == S.compute_contrast_factor(imgs[i], 0.7, 1.0, 300), i
        want = fed_stated(imgs[i], flows[i], FED_TAUS[:7])[-1]
        same(lt[i], want[0], ("Lt", i))
        same(step[i], want[1], ("Lstep", i))
        exp = S.detector_response(imgs[i], 2)
        for name, v in exp.items():
            same(host(det[name])[i], v, (name, i))


# ---- whole extractions ------------------------------------------------------------------------------------------------------
def assert_is_statement(res, levels, contrast, how, img=0, what=None, bulk=True):
    """level info, tau bytes, the contrast factor and all ten planes of every level of image `img` of an extraction against the
    statement's; bulk: the planes through akz_fetch_pyramid (one call), else one akz_fetch_plane each"""
    assert res.counts(img)[0] == len(levels), what
    assert X.contrast_equal(res.contrast(img), contrast), (what, res.contrast(img), contrast)
    pyr = res.pyramid(img) if bulk else None
    for l, lv in enumerate(levels):
        info = res.level_info(l)
        for f in INFO:
            assert info[f] == lv[f], (what, l, f, info[f], lv[f])
        assert info["tau"].tobytes() == lv["tau"].tobytes(), (what, l)
        for p in S.PLANES:
            a, b = (pyr[l][p] if bulk else res.plane(l, p, img)), lv["planes"][p]
            assert a.shape == b.shape, (what, l, p, a.shape, b.shape)
            if not X.planes_equal(a, b, how):
                bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
                raise AssertionError(f"{what}: level {l} plane {p}: {len(bad)} words differ, first at {bad[0]}: "
                                     f"{a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}")


def device_f32(frames):
    """[N, H, W] u8 or f32 host frames as the f32 device batch of the begin / finish interface (image.rs:136 for u8)"""
    import torch
    frames = np.asarray(frames)
    return torch.from_numpy(S.unit_float(frames) if frames.dtype == np.uint8 else frames).cuda()


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_case_under_every_forced_row(ctx, amd, name):
    """every case of tests/scalespace_cases.py, all ten planes of every level, under every forced gate side: the synchronous
    call on the frame as it is (u8 where the case is) and extract_begin(...).finish() on the f32 frame"""
    import torch
    from test_gpu_gates import FORCED
    assert RESIDENT_ROW in [row[0] for row in FORCED]
    _, frame, kw, how = X.case(name)
    levels, contrast = X.stated(name)
    cfg = amd.Config(**kw)
    d_f32 = device_f32(frame[None])
    torch.cuda.synchronize()
    try:
        for label, force, undo in FORCED:
            force(ctx)
            try:
                cmp = how_under(name, how, label == RESIDENT_ROW)
                sync = ctx.extract_features(frame, cfg, keep_all_planes=True)
                assert_is_statement(sync, levels, contrast, cmp, what=(name, label, "synchronous"), bulk=label != "default")
                sync.close()
                asyn = ctx.extract_begin(d_f32, cfg, keep_all_planes=True).finish()
                assert_is_statement(asyn, levels, contrast, cmp, what=(name, label, "begin / finish"))
                asyn.close()
            finally:
                undo(ctx)
    finally:
        for _, _, undo in FORCED:
            undo(ctx)


@pytest.fixture(scope="module")
def rctx(amd):
    """prep mode 3, as tests/test_gpu_resident.py builds it: the marches and k_octave_resident wherever they are supported"""
    import torch
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    c.set_prep_mode(3)
    c.debug_set_host_sort(False)
    yield c
    c.close()


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_case_in_a_resident_context(rctx, amd, name):
    _, frame, kw, how = X.case(name)
    how = how_under(name, how, True)
    levels, contrast = X.stated(name)
    res = rctx.extract_features(frame, amd.Config(**kw), keep_all_planes=True)
    assert_is_statement(res, levels, contrast, how, what=(name, "prep mode 3"))
    res.close()
    res = rctx.extract_begin(device_f32(frame[None]), amd.Config(**kw), keep_all_planes=True).finish()
    assert_is_statement(res, levels, contrast, how, what=(name, "prep mode 3", "begin / finish"))
    res.close()


@pytest.mark.parametrize("w,h,n", [(163, 81, 3), (130, 66, 4)])
def test_batches_on_the_batch_and_the_lone_path(ctx, amd, w, h, n):
    """different frames in one job: every image's planes are its own, on the forced batch path and on the forced lone path"""
    import torch
    frames = np.stack([X.natural(w, h, 500 + i) for i in range(n)])
    want = [S.pyramid(f, X.config()) for f in frames]
    d_u8 = torch.from_numpy(frames).cuda()
    d_f32 = device_f32(frames)
    torch.cuda.synchronize()
    try:
        for label, value in (("batch path", 1), ("lone path", 2_000_000)):
            ctx.debug_set_schedule(4, value)
            for entry, res in (("synchronous", ctx.extract_features(d_u8, keep_all_planes=True)),
                               ("begin / finish", ctx.extract_begin(d_f32, keep_all_planes=True).finish())):
                for i in range(n):
                    assert_is_statement(res, want[i][0], want[i][1], "value", img=i, what=(label, entry, i))
                res.close()
    finally:
        ctx.debug_set_schedule(4, 0)


# ---- the chain and the bulk fetch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,idx,ch", CHAIN_FRAMES)
def test_extract_features_is_the_statement_chain(ctx, amd, w, h, idx, ch):
    """keypoints (every field, the angle's bits) and descriptor bytes of extract_features equal pyramid() ->
    extrema_numpy.detect -> mldb_numpy.describe, in the default mode and with selection and sort forced to the device"""
    frame = amd.synth_frame(w, h, idx)
    kps, desc, levels, contrast = S.extract(frame, X.config(descriptor_channels=ch))
    assert len(kps) >= 15
    cfg = amd.Config(descriptor_channels=ch)
    try:
        for label in ("default", "device selection and sort"):
            if label != "default":
                ctx.debug_set_select(2)
                ctx.debug_set_host_sort(False)
            res = ctx.extract_features(frame, cfg, keep_all_planes=True)
            got = res.keypoints()
            assert len(got) == len(kps), (label, len(got), len(kps))
            for f in KP_FIELDS:
                a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(kps[f])
                if a.dtype.kind == "f":
                    a, b = a.view(np.uint32), b.view(np.uint32)
                assert np.array_equal(a, b), (label, f)
            assert np.array_equal(res.descriptors(), desc), label
            assert_is_statement(res, levels, contrast, "value", what=(w, h, idx, label))
            res.close()
    finally:
        ctx.debug_set_select(None)
        ctx.debug_set_host_sort(None)


@pytest.mark.parametrize("keep", [True, False], ids=["all", "lean"])
def test_bulk_fetch_returns_the_statements_planes(ctx, amd, keep):
    """akz_fetch_pyramid, the call the Rust shim downloads a pyramid with: into a caller's buffer, kept planes and the ones a
    lean result recomputes on fetch alike; and plane by plane through akz_fetch_plane"""
    _, frame, kw, how = X.case("322x200")
    levels, contrast = X.stated("322x200")
    res = ctx.extract_features(frame, amd.Config(**kw), keep_all_planes=keep)
    out = np.full(res.pyramid_floats() + 3, np.nan, np.float32)
    pyr = res.pyramid(out=out)
    assert np.isnan(out[-3:]).all() and not np.isnan(out[:-3]).any()
    for l, lv in enumerate(levels):
        for p in S.PLANES:
            assert X.planes_equal(pyr[l][p], lv["planes"][p], how), (l, p)
    assert_is_statement(res, levels, contrast, how, what="bulk", bulk=True)
    assert_is_statement(res, levels, contrast, how, what="plane by plane", bulk=False)
    res.close()
