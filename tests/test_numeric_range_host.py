"""The premises of tests/test_gpu_numeric_range.py, on the oracle alone (no GPU): the regimes of tests/range_cases.py really
put the planes where their names say, the oracle's planes and contrast factor are exactly power-of-two equivariant between
the regimes that stay normal, and the per-op inputs at the crossing exponents really give subnormal outputs."""
import numpy as np
import pytest

import range_cases as R


@pytest.fixture(scope="module", autouse=True)
def drop_cached_oracle_results():
    """the shared oracle results are freed with the module, not at interpreter exit"""
    yield
    R.oracle_result.cache_clear()


@pytest.fixture(scope="module")
def amd_host():
    """the product binding for its host utilities (synth_frame, plan_levels): no GPU needed"""
    import akaze_amd
    akaze_amd.lib()
    return akaze_amd


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
def test_frame_shapes_have_three_octaves_of_levels_at_least_16_px(amd_host, shape):
    w, h, _ = shape
    levels = amd_host.plan_levels(w, h)
    assert max(lv["octave"] for lv in levels) >= 2
    assert all(lv["w"] >= 16 and lv["h"] >= 16 for lv in levels)
    # no smaller frame of this kind has the third octave (evolution.rs:138-149 admits it at 80 x 40)
    assert max(lv["octave"] for lv in amd_host.plan_levels(w - 8, h)) < 2 and max(lv["octave"] for lv in amd_host.plan_levels(w, h - 4)) < 2
    if w % 8 == 0:
        assert all(lv["w"] % 8 == 0 for lv in levels)
    else:
        assert all(lv["w"] % 8 for lv in levels) and any(lv["h"] % 2 for lv in levels)


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
@pytest.mark.parametrize("regime", list(R.REGIME_CONDITIONS))
def test_regime_conditions_hold_on_the_oracle(ref, amd_host, regime, shape):
    rf = R.oracle_result(ref, amd_host, shape, regime)
    shares = {n: (round(max(R.subnormal_share(p) for p in R.all_levels(rf, n)), 3),
                  round(R.zero_share(np.concatenate([p.ravel() for p in R.all_levels(rf, n)])), 3)) for n in ("Lt", "Lx", "Lxx", "Lstep", "Ldet")}
    print(f"{regime} {shape[0]}x{shape[1]} e={R.REGIMES[regime]}: {rf.num_keypoints} keypoints, contrast {rf.contrast:.3g}, "
          f"(best level's subnormal share, zero share) {shares}")
    assert R.REGIME_CONDITIONS[regime](rf), shares


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
def test_oracle_keypoints_survive_where_the_gpu_tests_need_them(ref, amd_host, shape):
    """natural and small_normal detect the same extrema; the responses of ldet_subnormal are themselves subnormal"""
    n0 = R.oracle_result(ref, amd_host, shape, "natural").num_keypoints
    assert n0 > 500 and R.oracle_result(ref, amd_host, shape, "small_normal").num_keypoints == n0
    resp = R.oracle_result(ref, amd_host, shape, "ldet_subnormal").keypoints()["response"]
    assert len(resp) >= 10 and R.subnormal_share(resp) == 1.0


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=R.FRAME_IDS)
@pytest.mark.parametrize("regime", ["small_normal", "large"])
def test_oracle_planes_and_contrast_are_power_of_two_equivariant(ref, amd_host, regime, shape):
    """Multiplying the frame by 2^e multiplies Ldet by 2^2e, leaves Lflow alone and multiplies every other plane and the
    contrast factor by 2^e, exactly, as long as nothing leaves the normal range: the premise of the oracle-free GPU check."""
    e = R.REGIMES[regime]
    nat, rf = R.oracle_result(ref, amd_host, shape, "natural"), R.oracle_result(ref, amd_host, shape, regime)
    assert rf.contrast == np.ldexp(nat.contrast, e)
    for lvl in range(nat.num_levels):
        for name in R.PLANES:
            a, b = nat.plane(lvl, name), rf.plane(lvl, name)
            assert a.shape == b.shape
            if a.size:
                want = np.ldexp(a, R.PLANE_EXPONENT[name] * e)
                assert want.dtype == np.float32 and np.array_equal(want, b), (lvl, name)
                assert R.subnormal_share(b) == 0.0 and np.isfinite(b).all()


def _shares(fn, shapes=None):
    return [round(R.subnormal_share(fn(shape)), 3) for shape in shapes or R.OP_SHAPES + [R.STRIP_SHAPE]]


def test_op_outputs_are_subnormal_at_the_crossing_exponents(ref):
    """more than 25 % of the oracle's output is nonzero subnormal at every exponent of R.CROSSING, on every shape"""
    kern = np.random.default_rng(10).standard_normal(9).astype(np.float32)
    rows = {}
    for e in R.CROSSING["filter"]:
        rows["horizontal_filter", e] = _shares(lambda s: ref.horizontal_filter(R.op_plane(s, 1, e), kern))
        rows["vertical_filter", e] = _shares(lambda s: ref.vertical_filter(R.op_plane(s, 1, e), kern))
    for e in R.CROSSING["gaussian_blur"]:
        for sigma in (1.0, 1.6, 2.5):
            rows["gaussian_blur", sigma, e] = _shares(lambda s: ref.gaussian_blur(R.op_plane(s, 2, e), sigma))
    for e in R.CROSSING["half_size"]:
        rows["half_size", e] = _shares(lambda s: ref.half_size(R.op_plane(s, 3, e)))
    for e in R.CROSSING["scharr"]:
        for sigma in range(1, 7):
            rows["scharr x", sigma, e] = _shares(lambda s: ref.scharr(R.op_plane(s, 4, e), True, False, sigma))
            rows["scharr y", sigma, e] = _shares(lambda s: ref.scharr(R.op_plane(s, 4, e), False, True, sigma))
    for e in R.CROSSING["detector_response"]:
        for sigma in range(1, 7):
            rows["Ldet", sigma, e] = _shares(lambda s: R.detector_expected(ref, R.op_plane(s, 60 + sigma, e), sigma)["Ldet"])
    for ek in R.CROSSING["pm_g2_k"]:
        k = 0.0123 * 2.0 ** ek
        rows["pm_g2", ek] = _shares(lambda s: ref.pm_g2(R.op_plane(s, 5, 0), R.op_plane(s, 6, 0), k))
        rows["flow", ek] = _shares(lambda s: ref.pm_g2(ref.scharr(R.op_plane(s, 7, 0), True, False, 1),
                                                      ref.scharr(R.op_plane(s, 7, 0), False, True, 1), k))
    for e in R.CROSSING["fed_steps"]:
        for tiny in (False, True):
            rows["fed Lt", tiny, e] = _shares(lambda s: R.fed_expected(ref, R.op_plane(s, 9, e), R.fed_flow(s, 10, tiny), R.FED_TAUS)[0],
                                             R.FED_SHAPES)
    for key, shares in rows.items():
        print(key, shares)
    assert all(min(shares) > 0.25 for shares in rows.values()), {k: v for k, v in rows.items() if min(v) <= 0.25}


def test_contrast_inputs_straddle_the_f32_underflow_of_the_squared_gradient(ref):
    """What a kernel that squared the gradient in f32 would see: all normal at the top of R.CONTRAST_EXPS, subnormal in
    between, all zero at the bottom -- while the oracle's contrast factor (squared in f64) stays exactly 2^e-equivariant
    wherever the gradients themselves are normal."""
    shape = R.OP_SHAPES[2]
    imgs = R.contrast_images(ref, shape, R.CONTRAST_EXPS)
    sub, zero = {}, {}
    for e, img in zip(R.CONTRAST_EXPS, imgs):
        b = ref.gaussian_blur(img, 1.0)
        gx, gy = ref.scharr(b, True, False, 1), ref.scharr(b, False, True, 1)
        with np.errstate(under="ignore", over="ignore"):
            ss = gx * gx + gy * gy
        sub[e], zero[e] = R.subnormal_share(ss), R.zero_share(ss)
        k = ref.contrast_factor(img, 0.7, 1.0, 300)
        assert np.isfinite(k) and k > 0.0 and k != 0.03, (e, k)
    print(sub, zero)
    assert sub[0] == zero[0] == 0.0 and sub[-62] > 0.9 and 0.0 < zero[-68] < 0.5 and zero[-74] == 1.0 and zero[-140] == 1.0
    for batch in R.CONTRAST_BATCHES:
        assert set(batch) <= set(R.CONTRAST_EXPS) and max(batch) - min(batch) >= 100  # (30 orders of magnitude and more)
