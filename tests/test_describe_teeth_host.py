"""The describe cases (tests/describe_cases.py) have teeth: every mutation switch of the numpy statement of the two keypoint
ops (tests/mldb_numpy.py) changes the angle or the descriptor row of at least 10 keypoints of the cases CATCHES names for it,
no case is idle, the two switches that no input can catch are proven to be such, and the oracle agrees with the unmutated
statement on the tie and mirror families.  Statement against statement (and against the oracle): the product has no say, so
the test says what tests/test_gpu_describe.py can tell apart, on the very planes and keypoints it sends through the kernels.
No GPU.

A case is family-WxH-channels-orient|given: `orient` computes the orientation, `given` keeps the keypoint's angle."""
import functools

import numpy as np
import pytest

import describe_cases as D
import extrema_numpy as E
import mldb_numpy as M

MIN_KEYPOINTS = 10

# per switch, the cases that MUST change for at least MIN_KEYPOINTS keypoints under it.  The expression-order, division and
# square-root switches are held by tie or mirror cases at every channel count they apply to: the crafted planes catch them by
# luck or not at all (desc_sqrt_f64: 0 keypoints of every crafted case).
WIDE_O, WIDE_2, WIDE_1 = "wide-64x40-3ch-orient", "wide-64x40-2ch-given", "wide-64x40-1ch-given"
TIE = tuple(f"tie-163x81-{ch}ch-given" for ch in (3, 2, 1))
MIRROR = tuple(f"mirror-163x81-{ch}ch-given" for ch in (3, 2, 1))
CATCHES = {
    "ori_disc_le": (WIDE_O,), "ori_angs_yx": (WIDE_O,), "ori_sums_reset": (WIDE_O,), "ori_no_wrap": (WIDE_O,),
    "ori_best_ge": (WIDE_O, "flat_gradients-64x40-3ch-orient", "ly_not_positive-64x40-3ch-orient"),
    "ori_last_window_off": (WIDE_O,), "ori_j_outer": (WIDE_O,), "ori_lx_ly_swapped": (WIDE_O,), "ori_scale_trunc": (WIDE_O,),
    "ori_weight_off_x": (WIDE_O,), "ori_final_xy": (WIDE_O,), "ori_keypoint_octave": (WIDE_O,),
    "round_half_even": (WIDE_O, TIE[2]),
    "desc_ge": ("ints-64x40-2ch-given", MIRROR[0]),
    "desc_no_half": (WIDE_2,),
    "desc_left_assoc": (WIDE_2, TIE[0]),
    "desc_hoist": TIE,
    "desc_fused": TIE,
    "desc_kl_swapped": MIRROR,
    "desc_cells_j_outer": (WIDE_2,),
    "desc_step_floor": (WIDE_2,),
    "desc_scale_trunc": (WIDE_1,),
    "desc_dxdy_swapped": (MIRROR[0], TIE[0]),
    "desc_rot_sign": (WIDE_2,),
    "desc_channel_minor": (WIDE_2, MIRROR[0]),
    "desc_msb_first": (WIDE_1,),
    "desc_no_div": MIRROR,
    "desc_recip": MIRROR,
    "desc_sqrt_f64": (MIRROR[1],),
    "desc_level_octave": (WIDE_1,),
}

# the cases of the 64 x 40 pyramid as tests/test_gpu_describe.py runs them (family, channels), each of which has to change under
# at least one switch; with the given angle, which is the cheaper half of a case (CATCHES holds orient cases of three kinds)
SMALL = [f"{k}-64x40-{ch}ch-given" for k in D.KINDS for ch in ((3, 1, 2) if k == "wide" else (3, 2) if k == "ints" else (3,))] + \
        [f"{k}-64x40-{ch}ch-given" for k in ("tie", "mirror") for ch in (3, 2, 1)]
PROBES = ("desc_ge", "desc_msb_first")
ORIENT = [f"{k}-64x40-3ch-orient" for k in D.KINDS]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def levels(w, h):
    return tuple(dict(w=lw, h=lh, octave=o, esigma=e) for lw, lh, o, e in E.plan_levels(w, h))


@functools.lru_cache(maxsize=None)
def inputs(family, w, h, ch):
    """(planes as the statement takes them, octaves, keypoints, meta) -- seeds as in tests/test_gpu_describe.py"""
    lv = levels(w, h)
    meta = None
    if family == "tie":
        src = D.crafted_planes(lv, "wide", seed=w + 11)
        kps, meta = D.tie_keypoints(lv, src, seed=w + 12)
    elif family == "mirror":
        src = D.mirror_planes(lv, seed=w + 13)
        kps, meta = D.mirror_keypoints(lv)
    else:
        src = D.crafted_planes(lv, family, seed=w * 7 + ch)
        kps = D.crafted_keypoints(lv)
    return D.as_tuples(src), [l["octave"] for l in lv], kps, meta


def parse(case):
    family, size, ch, orient = case.rsplit("-", 3)
    w, h = size.split("x")
    return family, int(w), int(h), int(ch[0]), orient == "orient"


@functools.lru_cache(maxsize=None)
def stated(case, mut=()):
    family, w, h, ch, orient = parse(case)
    planes, octaves, kps, _ = inputs(family, w, h, ch if family in D.KINDS else 0)
    a, d, _ = M.describe(planes, octaves, kps, ch, "clamped", orient, mut)
    return a, d


def angles(case, mut):
    """the orientation alone (what an ori_* switch can touch), level by level as M.describe goes"""
    family, w, h, ch, orient = parse(case)
    planes, octaves, kps, _ = inputs(family, w, h, ch if family in D.KINDS else 0)
    assert orient
    out = np.zeros(len(kps), np.float32)
    for l in range(len(planes)):
        sel = kps["class_id"] == l
        out[sel] = M.main_orientation(planes[l][1], planes[l][2], octaves[l], kps[sel], "clamped", mut=mut)
    return out


def changed(case, switch):
    """the number of keypoints of the case whose angle word or descriptor row is another under the switch (under an ori_*
    switch: whose angle word is another; the descriptor is not asked, it could only add keypoints)"""
    a0, d0 = stated(case)
    if switch.startswith("ori_"):
        return int((bits(a0) != bits(angles(case, (switch,)))).sum())
    a1, d1 = stated(case, (switch,))
    return int(((bits(a0) != bits(a1)) | (d0 != d1).any(axis=1)).sum())


def test_levels_are_the_librarys(amd):
    for w, h in ((163, 81), (64, 40), (517, 389)):
        plan = amd.plan_levels(w, h)
        assert [(p["w"], p["h"], p["octave"], p["esigma"]) for p in plan] == [(l["w"], l["h"], l["octave"], l["esigma"]) for l in levels(w, h)]


def test_unknown_switch_is_refused():
    with pytest.raises(AssertionError):
        M.describe([], [], np.zeros(0, M.KEYPOINT_DTYPE), 3, "clamped", True, ("desc_gt",))
    assert set(M.INVISIBLE) < set(M.SWITCHES) and len(set(M.SWITCHES)) == len(M.SWITCHES)


@pytest.mark.parametrize("switch", [s for s in M.SWITCHES if s not in M.INVISIBLE])
def test_switch_is_caught(switch):
    """statement against mutated statement on the cases CATCHES names: at least MIN_KEYPOINTS keypoints change in each"""
    assert set(CATCHES) == set(M.SWITCHES) - set(M.INVISIBLE)
    assert CATCHES[switch]
    for case in CATCHES[switch]:
        n = changed(case, switch)
        print(f"{switch:20s} {case:32s} {n:5d} of {len(stated(case)[0])} keypoints change")
        assert n >= MIN_KEYPOINTS, (switch, case, n)


def test_fine_switches_are_held_by_tie_and_mirror_cases():
    """not by luck on `wide`: the switches a faster k_mldb is likely to trip are named against the families built for them,
    at every channel count at which they can show"""
    for s in ("desc_hoist", "desc_fused", "desc_no_div", "desc_recip", "desc_kl_swapped"):
        for ch in (3, 2, 1):
            assert any(parse(c)[0] in ("tie", "mirror") and parse(c)[3] == ch for c in CATCHES[s]), (s, ch)
    assert any(parse(c)[0] in ("tie", "mirror") and parse(c)[3] == 2 for c in CATCHES["desc_sqrt_f64"])  # (2 channels only)


@pytest.mark.parametrize("case", SMALL)
def test_no_case_is_idle(case):
    hit = next((s for s in PROBES if changed(case, s)), None)
    print(f"{case:32s} changes under {hit}")
    assert hit, case


def test_tie_and_mirror_cases_are_what_they_claim():
    for w, h in ((163, 81), (64, 40)):
        _, _, kps, meta = inputs("tie", w, h, 0)
        apart = D.tie_rounds_apart(kps, meta)
        print(f"tie {w}x{h}: {int(apart.sum())} of {len(kps)} keypoints have a sample that two associations round apart")
        assert apart.all() and len(kps) == 64 * len(levels(w, h))
        assert set(np.round(0.5 * kps["size"] / 2.0 ** kps["octave"].astype(float))) == set(D.TIE_SCALES)
        assert len(set(kps["angle"]) & set(np.array(D.SPECIAL_ANGLES, np.float32))) >= 3  # special angles among them
        planes, octaves, kps, meta = inputs("mirror", w, h, 0)
        for ch in (3, 2, 1):
            if w == 64:  # (163 x 81: test_oracle_equals_statement_on_mirror_and_tie_keypoints asserts the same)
                ref_a, ref_d, rcov = M.describe(planes, octaves, kps, ch, "reference", False)
                assert rcov.completes.all() and not rcov.next_row.any()      # every sample inside the plane
                assert np.array_equal(ref_d, stated(f"mirror-{w}x{h}-{ch}ch-given")[1])
            vals = np.zeros((29, 3, len(kps)), np.float32)
            for l in range(len(planes)):
                sel = kps["class_id"] == l
                vals[:, :, sel] = M.mldb_values(*planes[l], kps[sel], kps["angle"][sel], ch, "clamped")
            pairs, close, tied = D.mirror_closeness(vals, meta, ch)
            print(f"mirror {w}x{h} {ch}ch: {pairs} mirrored cell pairs, {close} with means within 4 ulp, {tied} equal")
            assert 2 * close >= pairs and tied >= 100


def _in_window(ang1, ang2, two_pi, ang, le):
    """scale_space_extrema.rs:313-314 for one positive angle, with `<` or `<=` at the edges"""
    lt = (lambda a, b: a <= b) if le else (lambda a, b: a < b)
    return bool((ang1 < ang2 and lt(ang1, ang) and lt(ang, ang2)) or (ang2 < ang1 and (lt(ang, ang2) or (lt(ang1, ang) and lt(ang, two_pi)))))


def test_the_two_invisible_switches_are_invisible():
    """ori_edges_f64 and ori_edges_le cannot be caught by ANY input, and this is why (tests/mldb_numpy.py's docstring): the
    sample angles are atan2f(res_y, res_y), which takes five words and NaN; only pi/4 is positive; and pi/4 is no window edge
    and lies in the same windows however the edges are accumulated or compared.  Then they change nothing on the cases."""
    F = np.float32
    pi4 = F(np.pi / 4)
    allowed = set(bits(np.array([pi4, -3 * pi4, 0.0, -0.0, -np.pi], F)).tolist())
    weights = np.unique(M.GAUSS25)
    probes = [np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 1.0, -1.0, 3e38, -3e38, np.inf, -np.inf, np.nan], F)]
    for family, w, h, ch in {parse(c)[:4] for c in SMALL + ORIENT} | {("tie", 163, 81, 3), ("mirror", 163, 81, 3)}:
        probes += [p[2].ravel() for p in inputs(family, w, h, ch if family in D.KINDS else 0)[0]]
    with np.errstate(all="ignore"):
        for ly in probes:
            for g in weights:
                res_y = g * ly
                a = M.atan2f(res_y, res_y)
                assert set(bits(a[~np.isnan(a)]).tolist()) <= allowed
    w32, w64 = M.orientation_windows(), M.orientation_windows(np.float64)
    assert len(w32) == len(w64) == 42
    member = []
    for T, ws in ((F, w32), (np.float64, w64)):
        two_pi, ang = T(2.0) * T(M.PI), T(pi4)
        assert all(T(a1) != ang and T(a2) != ang for a1, a2 in ws) and two_pi != ang   # pi/4 is no edge: `<=` is `<`
        for le in (False, True):
            member.append([_in_window(a1, a2, two_pi, ang, le) for a1, a2 in ws])
    assert all(m == member[0] for m in member) and 0 < sum(member[0]) < 42           # the same windows hold pi/4
    for case in ORIENT:
        for s in M.INVISIBLE:
            assert changed(case, s) == 0, (case, s)


@functools.lru_cache(maxsize=None)
def large_ties():
    """tie keypoints searched on a 517 x 389 pyramid of wide planes, where the lattices of scale 3 to 7 fit inside"""
    lv = levels(517, 389)
    src = D.crafted_planes(lv, "wide", seed=528)
    return src, D.tie_keypoints(lv, src, seed=529, per_slot=1)[0]


@pytest.mark.parametrize("ch", [3, 2, 1])
def test_oracle_equals_statement_on_mirror_and_tie_keypoints(ref, ch):
    """The oracle has an entry that takes a caller's planes (ref_detect_from_planes; Ldet zero: no keypoints of its own).  It
    is asked about the mirror keypoints of 163 x 81 -- with the given angle all of them -- and about tie keypoints of a
    517 x 389 pyramid: those for which the statement's reference form says that every read stays inside the plane (the
    oracle's reads are unchecked).  With the given angle at every channel count, with the orientation at 3 channels."""
    for family, w, h, least in (("mirror", 163, 81, (576, 200)), ("tie", 517, 389, (100, 100))):
        lv = levels(w, h)
        if family == "tie":
            src, kps = large_ties()
        else:
            planes, _, kps, _ = inputs(family, w, h, 0)
            src = [dict(Lt=p[0], Lx=p[1], Ly=p[2]) for p in planes]
        planes, octaves = D.as_tuples(src), [l["octave"] for l in lv]
        rf = ref.detect_from_planes(w, h, [dict(p, Ldet=np.zeros_like(p["Lt"])) for p in src], ref.default_config(descriptor_channels=ch))
        assert rf.num_keypoints == 0 and rf.num_levels == len(lv)
        for orient in (False, True) if ch == 3 else (False,):
            ang, desc, cov = M.describe(planes, octaves, kps, ch, "reference", orient)
            ask = np.nonzero(cov.completes & ~cov.next_row)[0]
            print(f"{family} {w}x{h} {ch}ch orient={orient}: the oracle is asked about {len(ask)} of {len(kps)} keypoints")
            assert len(ask) >= least[orient]   # (mirror, given angle: all of them)
            k_or, d_or = rf.describe(kps[ask], compute_orientation=orient)
            assert np.array_equal(bits(k_or["angle"]), bits(ang[ask])) and np.array_equal(d_or, desc[ask]), (family, orient)
        rf.close()
