"""k_orientation and k_mldb as stand-alone ops on keypoints the detector did NOT produce (akz_result_describe_keypoints:
ops::scale_space_extrema::compute_main_orientation, ops::descriptors::extract_descriptors): at and beyond the border, on
every level, with octaves that are not their level's, at degenerate scales and angles, with non-finite fields, at every
keypoint count around the kernels' workgroup sizes, on every image of a batch and with 1 / 2 / 3 channels; and on the two
families built so that a NEARLY right kernel goes wrong, tie keypoints and mirror planes (the planes and keypoints are
tests/describe_cases.py's; tests/test_describe_teeth_host.py proves which deviations they catch).

Expected values come from tests/mldb_numpy.py -- a numpy statement of the two ops written from the reference's text and held
to the oracle by tests/test_describe_host.py -- in its `clamped` form, the product's contract.  Where the statement says that
the reference itself completes and its `reference` form gives the same words, the answer is the reference's too; the tests
print how often.  No tolerance anywhere: float words and descriptor bytes are compared for equality, for every keypoint
generated (none is filtered out)."""
import numpy as np
import pytest

import describe_cases as D
import mldb_numpy as M

SIZES = [(517, 389), (163, 81), (64, 40)]
KINDS = D.KINDS
INVALID_ARG = -1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def crafted_planes(amd, w, h, kind, seed):
    return D.crafted_planes(amd.plan_levels(w, h), kind, seed)


crafted_keypoints, nonfinite_keypoints = D.crafted_keypoints, D.nonfinite_keypoints


def upload(ctx, amd, w, h, planes, ch):
    res = ctx.extract_from_planes(w, h, planes, amd.Config(descriptor_channels=ch), detect=False)
    assert res.counts() == (len(planes), 0, (162 * ch + 7) // 8)
    return res


def result_planes(res, n_levels, img=0):
    """the planes the result itself holds, and the octaves of its levels: what the statement is given"""
    planes = [tuple(res.plane(l, p, img) for p in ("Lt", "Lx", "Ly")) for l in range(n_levels)]
    return planes, [res.level_info(l)["octave"] for l in range(n_levels)]


def assert_rows(got_k, got_d, kps, exp_a, exp_d, what):
    bad_a = np.nonzero(bits(got_k["angle"]) != bits(exp_a))[0]
    bad_d = np.nonzero((got_d != exp_d).any(axis=1))[0]
    print(f"{what}: {len(kps)} keypoints, {len(bad_a)} angles and {len(bad_d)} descriptors differ")
    assert len(bad_a) == 0 and len(bad_d) == 0, (what, bad_a[:8], kps[bad_a[:3]], bad_d[:8], kps[bad_d[:3]])
    for f in ("x", "y", "response", "size", "octave", "class_id"):  # the call writes the angle, nothing else
        assert got_k[f].tobytes() == kps[f].tobytes(), (what, f)


CASES = [(s, k, ch) for s in SIZES for k in KINDS for ch in ((3, 1, 2) if k == "wide" else (3, 2) if k == "ints" else (3,))]


@pytest.mark.gpu
@pytest.mark.parametrize("size,kind,ch", CASES, ids=[f"{s[0]}x{s[1]}-{k}-{ch}ch" for s, k, ch in CASES])
def test_crafted_planes_and_keypoints(ctx, amd, size, kind, ch):
    w, h = size
    src = crafted_planes(amd, w, h, kind, seed=w * 7 + ch)
    res = upload(ctx, amd, w, h, src, ch)
    planes, octaves = result_planes(res, len(src))
    for l, p in enumerate(src):
        assert all(planes[l][i].tobytes() == p[n].tobytes() for i, n in enumerate(("Lt", "Lx", "Ly"))), l
    kps = crafted_keypoints(amd.plan_levels(w, h))
    assert len(kps) == 540 * len(src) and set(kps["class_id"]) == set(range(len(src)))
    for orient in (True, False):
        what = f"{w}x{h} {kind} {ch}ch orient={orient}"
        got_k, got_d = res.describe_keypoints(kps, compute_orientation=orient)
        assert got_d.shape == (len(kps), (162 * ch + 7) // 8)
        exp_a, exp_d, cov = M.describe(planes, octaves, kps, ch, "clamped", orient)
        assert_rows(got_k, got_d, kps, exp_a, exp_d, what)
        if not orient or kind in ("flat_gradients", "ly_not_positive"):
            assert bits(got_k["angle"]).tobytes() == bits(kps["angle"]).tobytes(), what  # the given angle, -0.0 and 1000.0 included
        # the border cases are border cases (from the statement's side alone)
        sides = {s: int(getattr(cov, s).sum()) for s in ("left", "right", "top", "bottom")}
        ref_a, ref_d, rcov = M.describe(planes, octaves, kps, ch, "reference", orient)
        wrapped = rcov.completes & rcov.next_row
        also_reference = rcov.completes & (bits(ref_a) == bits(exp_a)) & (ref_d == exp_d).all(axis=1)
        print(f"{what}: clamped samples {sides}; the reference completes for {int(rcov.completes.sum())}, "
              f"{int(wrapped.sum())} of them through the next row; {int(also_reference.sum())} answers are the reference's too")
        assert min(sides.values()) >= 50 and wrapped.sum() >= 50, (what, sides, int(wrapped.sum()))
        assert also_reference[rcov.completes & ~rcov.next_row].all()  # in-plane samples only: the two forms are one
    if kind == "ints":  # exact ties between cell means exist, so `>` is told from `>=`
        k0 = kps[kps["class_id"] == 0]
        v = M.mldb_values(*planes[0], k0, k0["angle"], ch, "clamped")
        ties = sum(int((v[a, 0] == v[b, 0]).sum()) for a in range(13, 29) for b in range(a + 1, 29))
        print(f"{w}x{h} ints {ch}ch: {ties} exact ties among the 4x4 grid's intensity means of level 0")
        assert ties >= 100
    res.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [3, 2])
def test_non_finite_keypoints_follow_the_clamped_form(ctx, amd, ch):
    """NaN, the infinities and 1e30 as x, y, size and angle.  Every gather index of both kernels is clamped AFTER the
    float-to-int conversion (v_cvt_i32_f32, which saturates and turns NaN into 0, then v_min_i32 with the plane's size - 1
    and a select of 0 for negatives, in the gfx950 code of k_orientation and k_mldb: DESIGN.md), so these cannot leave
    the planes; what they give is the statement's clamped form."""
    w, h = 163, 81
    src = crafted_planes(amd, w, h, "wide", seed=99)
    res = upload(ctx, amd, w, h, src, ch)
    planes, octaves = result_planes(res, len(src))
    kps = nonfinite_keypoints(amd.plan_levels(w, h))
    assert len(kps) == 26 * len(src)
    for orient in (True, False):
        got_k, got_d = res.describe_keypoints(kps, compute_orientation=orient)
        exp_a, exp_d, _ = M.describe(planes, octaves, kps, ch, "clamped", orient)
        assert_rows(got_k, got_d, kps, exp_a, exp_d, f"non-finite {ch}ch orient={orient}")
    res.close()


@pytest.fixture(scope="module")
def counted(ctx, amd):
    """a 163 x 81 pyramid of wide planes, 257 crafted keypoints spread over all levels, and the statement's answer"""
    w, h = 163, 81
    src = crafted_planes(amd, w, h, "wide", seed=5)
    res = upload(ctx, amd, w, h, src, 3)
    planes, octaves = result_planes(res, len(src))
    kps = crafted_keypoints(amd.plan_levels(w, h))
    kps = kps[:: len(kps) // 257][:257].copy()
    assert len(kps) == 257 and len(set(kps["class_id"])) == len(src)
    exp_a, exp_d, cov = M.describe(planes, octaves, kps, 3, "clamped", True)
    assert (cov.left | cov.right | cov.top | cov.bottom).sum() > 100
    yield res, kps, exp_a, exp_d, (planes, octaves)
    res.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 31, 32, 33, 257])
def test_keypoint_counts_around_the_workgroup_sizes(counted, n):
    """4 keypoints per k_mldb workgroup, 32 per k_orientation workgroup, grids rounded up to 8 workgroups: the first n of
    the list and the LAST n (so that keypoint 0 is not always the same one)"""
    res, kps, exp_a, exp_d, _ = counted
    for sl in (slice(0, n), slice(257 - n, 257)):
        got_k, got_d = res.describe_keypoints(kps[sl], compute_orientation=True)
        assert_rows(got_k, got_d, kps[sl], exp_a[sl], exp_d[sl], f"n={n} {sl}")


@pytest.mark.gpu
def test_no_keypoints_and_twenty_thousand(counted, amd):
    res, kps, exp_a, exp_d, (planes, octaves) = counted
    L = amd.lib()
    assert L.akz_result_describe_keypoints(res._h, 0, None, 0, 1, None) == 0  # n = 0: null pointers accepted
    k0, d0 = res.describe_keypoints(kps[:0])
    assert len(k0) == 0 and d0.shape == (0, 61)
    n = 20003  # neither a multiple of 4 nor of 32; row i is row i mod 257 of the list checked against the statement
    idx = np.arange(n) % 257
    big = kps[idx].copy()
    got_k, got_d = res.describe_keypoints(big, compute_orientation=True)
    assert_rows(got_k, got_d, big, exp_a[idx], exp_d[idx], f"n={n}")
    # and a smaller call after the large one (the buffers are reused)
    got_k, got_d = res.describe_keypoints(kps[:5], compute_orientation=False)
    a5, d5, _ = M.describe(planes, octaves, kps[:5], 3, "clamped", False)
    assert_rows(got_k, got_d, kps[:5], a5, d5, "n=5 after n=20003")
    assert got_k.tobytes() == kps[:5].tobytes()


@pytest.mark.gpu
def test_every_image_of_a_batch_against_its_own_planes(ctx, amd):
    """kp.img > 0 (the kernels' ioff = img * stride): one keypoint list, border cases included, on the three images of a
    batch of different frames"""
    import torch
    w, h = 320, 240
    frames = np.stack([amd.synth_frame(w, h, 40 + i) for i in range(3)])
    res = ctx.extract_features(torch.from_numpy(frames).cuda())
    assert res.num_images == 3
    levels = amd.plan_levels(w, h)
    kps = crafted_keypoints(levels)[::5].copy()
    answers = []
    for img in range(3):
        planes, octaves = result_planes(res, len(levels), img)
        got_k, got_d = res.describe_keypoints(kps, img=img, compute_orientation=True)
        exp_a, exp_d, cov = M.describe(planes, octaves, kps, 3, "clamped", True)
        assert_rows(got_k, got_d, kps, exp_a, exp_d, f"image {img} of 3")
        assert (cov.left | cov.right | cov.top | cov.bottom).sum() > 200
        answers.append((got_k["angle"].copy(), got_d))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert (answers[a][1] != answers[b][1]).any(axis=1).sum() > len(kps) // 2, (a, b)
        assert (bits(answers[a][0]) != bits(answers[b][0])).sum() > len(kps) // 4, (a, b)
    res.close()


@pytest.mark.gpu
def test_orientation_takes_the_levels_octave_the_descriptor_the_keypoints(ctx, amd, ref):
    """scale_space_extrema.rs:279 reads evolutions[class_id].octave, descriptors.rs:51 keypoint.octave.  Interior keypoints one
    octave above / below their level's, on a real frame's pyramid: the statement, the oracle and the product agree."""
    w, h = 517, 389
    frame = amd.synth_frame(w, h, 31)
    res, rf = ctx.extract_features(frame), ref.extract(frame)
    levels = amd.plan_levels(w, h)
    planes, octaves = result_planes(res, len(levels))
    rows = []
    for lvl, lv in enumerate(levels):
        o = lv["octave"]
        for delta in (1, -1):
            if o + delta < 0:
                continue
            # both ops stay inside the plane: see tests/test_describe_host.py
            hi_x, hi_y = ((lv["w"] - 14) // 2, (lv["h"] - 14) // 2) if delta > 0 else (lv["w"] - 18, lv["h"] - 18)
            for px in np.linspace(16, hi_x, 7):
                for py in np.linspace(16, hi_y, 5):
                    r = 2.0 ** (o + delta)
                    rows.append((np.float32(px) * r, np.float32(py + 0.5) * r, 0.0, 2.0 * r, o + delta, lvl, 0.6, 0))
    kps = np.array(rows, M.KEYPOINT_DTYPE)
    assert len(kps) == 35 * (2 * len(levels) - 4) and (kps["octave"] != np.array(octaves, np.uint64)[kps["class_id"]]).all()
    exp_a, exp_d, cov = M.describe(planes, octaves, kps, 3, "reference", True)
    assert cov.completes.all() and not cov.next_row.any()   # (the oracle's reads are unchecked)
    ork, ord_ = rf.describe(kps, compute_orientation=True)
    assert np.array_equal(bits(ork["angle"]), bits(exp_a)) and np.array_equal(ord_, exp_d)
    got_k, got_d = res.describe_keypoints(kps, compute_orientation=True)
    assert_rows(got_k, got_d, kps, exp_a, exp_d, "octave != the level's octave")
    # the given angle: only the descriptor runs, from the keypoint's octave
    got_k, got_d = res.describe_keypoints(kps, compute_orientation=False)
    exp_a, exp_d, _ = M.describe(planes, octaves, kps, 3, "reference", False)
    assert_rows(got_k, got_d, kps, exp_a, exp_d, "octave != the level's octave, given angle")
    # a list in which only ONE keypoint has an octave of its own
    lvl_oct = np.array(octaves, np.uint64)
    mixed = kps[:40].copy()
    mixed["octave"][1:] = lvl_oct[mixed["class_id"][1:]]
    got_k, got_d = res.describe_keypoints(mixed, compute_orientation=True)
    exp_a, exp_d, _ = M.describe(planes, octaves, mixed, 3, "clamped", True)
    assert_rows(got_k, got_d, mixed, exp_a, exp_d, "one keypoint with an octave of its own")
    res.close()


@pytest.mark.gpu
def test_refusals_leave_the_buffers_alone(counted, amd):
    res, kps, _, _, _ = counted
    L = amd.lib()
    n_levels = res.counts()[0]

    def call(k, img=0, null_list=False, null_desc=False):
        k = k.copy()
        before = k.tobytes()
        desc = np.full((len(k), 61), 0xA5, np.uint8)
        st = L.akz_result_describe_keypoints(res._h, img, None if null_list else k.ctypes.data, len(k), 1,
                                             None if null_desc else desc.ctypes.data)
        msg = L.akz_last_error().decode()
        assert k.tobytes() == before and (desc == 0xA5).all(), msg  # angles and descriptor buffer untouched
        return st, msg

    good = kps[:5]
    bad = good.copy()
    bad["class_id"][4] = n_levels                       # the last of five: the four before it are valid
    assert call(bad) == (INVALID_ARG, "akz_result_describe_keypoints: keypoint class_id / octave out of range")
    bad = good.copy()
    bad["octave"][4] = 31
    assert call(bad) == (INVALID_ARG, "akz_result_describe_keypoints: keypoint class_id / octave out of range")
    assert call(good, img=res.num_images) == (INVALID_ARG, "null result or image index out of range")
    assert call(good, null_list=True) == (INVALID_ARG, "akz_result_describe_keypoints: null argument")
    assert call(good, null_desc=True) == (INVALID_ARG, "akz_result_describe_keypoints: null argument")
    bad = good.copy()
    bad["octave"][4] = 30                               # the largest octave that is accepted
    desc = np.zeros((5, 61), np.uint8)
    assert L.akz_result_describe_keypoints(res._h, 0, bad.ctypes.data, 5, 1, desc.ctypes.data) == 0
    with pytest.raises(amd.AkazeError):
        res.describe_keypoints(good, img=res.num_images)


@pytest.mark.gpu
@pytest.mark.parametrize("ch,nb", [(1, 21), (2, 41), (3, 61)])
def test_binding_row_width_on_a_result_without_keypoints(ctx, amd, ch, nb):
    """Result.describe_keypoints sizes its rows from the result's config, also when the result has no keypoints of its own"""
    w, h = 64, 40
    src = crafted_planes(amd, w, h, "wide", seed=3)
    res = upload(ctx, amd, w, h, src, ch)
    planes, octaves = result_planes(res, len(src))
    kps = crafted_keypoints(amd.plan_levels(w, h))[::9].copy()
    got_k, got_d = res.describe_keypoints(kps, compute_orientation=True)
    assert got_d.shape == (len(kps), nb) and got_d.dtype == np.uint8
    exp_a, exp_d, _ = M.describe(planes, octaves, kps, ch, "clamped", True)
    assert_rows(got_k, got_d, kps, exp_a, exp_d, f"{ch} channels, {nb}-byte rows")
    if (162 * ch) % 8:  # the bits behind the last comparison stay zero
        assert not (got_d[:, -1] >> ((162 * ch) % 8)).any()
    res.close()


_FAMILY = {}


def family(amd, name, w, h):
    """(source planes, keypoints, meta) of a tie or mirror case, built once per size; one keypoint is dropped so that the
    count is a multiple neither of 4 (k_mldb's workgroup) nor of 32 (k_orientation's)"""
    if (name, w, h) not in _FAMILY:
        levels = amd.plan_levels(w, h)
        if name == "tie":
            src = D.crafted_planes(levels, "wide", seed=w + 11)
            kps, meta = D.tie_keypoints(levels, src, seed=w + 12)
        else:
            src = D.mirror_planes(levels, seed=w + 13)
            kps, meta = D.mirror_keypoints(levels)
        assert len(kps) % 4 == 0
        _FAMILY[(name, w, h)] = (src, kps[:-1].copy(), meta[:-1].copy())
    return _FAMILY[(name, w, h)]


FAMILY_CASES = [(n, s, ch) for n in ("tie", "mirror") for s in ((163, 81), (64, 40)) for ch in (3, 2, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,size,ch", FAMILY_CASES, ids=[f"{n}-{s[0]}x{s[1]}-{ch}ch" for n, s, ch in FAMILY_CASES])
def test_tie_keypoints_and_mirror_planes(ctx, amd, name, size, ch):
    """The inputs on which a nearly right kernel goes wrong (tests/describe_cases.py; tests/test_describe_teeth_host.py shows
    which deviations they catch): tie keypoints, one lattice sample of which is decided by the last bit of
    descriptors.rs:112-113 as written, and mirror planes, on which mirrored cells hold the same samples in the opposite
    order, so that comparisons are decided by the rounding of the sums and of the division.  Every float word and descriptor
    byte equals the statement's clamped form."""
    w, h = size
    src, kps, meta = family(amd, name, w, h)
    assert len(kps) % 4 and set(kps["class_id"]) == set(range(len(src)))
    res = upload(ctx, amd, w, h, src, ch)
    planes, octaves = result_planes(res, len(src))
    for l, p in enumerate(src):
        assert all(planes[l][i].tobytes() == p[n].tobytes() for i, n in enumerate(("Lt", "Lx", "Ly"))), l
    # the cases are what they claim, from the statement's side alone
    if name == "tie":
        apart = D.tie_rounds_apart(kps, meta)
        print(f"tie {w}x{h}: {int(apart.sum())} of {len(kps)} keypoints have a sample that two associations round apart")
        assert apart.all()
        assert all(((meta["coord"] == c) & (meta["sign"] == s) & (meta["variant"] == v)).sum() >= len(src)
                   for c in (0, 1) for s in (-1, 1) for v in range(len(D.TIE_VARIANTS)))
    else:
        vals = np.zeros((29, 3, len(kps)), np.float32)
        for l in range(len(src)):
            sel = kps["class_id"] == l
            vals[:, :, sel] = M.mldb_values(*planes[l], kps[sel], kps["angle"][sel], ch, "clamped")
        pairs, close, tied = D.mirror_closeness(vals, meta, ch)
        print(f"mirror {w}x{h} {ch}ch: {pairs} mirrored cell pairs, {close} with means within 4 ulp, {tied} equal")
        assert 2 * close >= pairs and tied >= 100
    for orient in (True, False):
        what = f"{name} {w}x{h} {ch}ch orient={orient}"
        got_k, got_d = res.describe_keypoints(kps, compute_orientation=orient)
        exp_a, exp_d, cov = M.describe(planes, octaves, kps, ch, "clamped", orient)
        assert_rows(got_k, got_d, kps, exp_a, exp_d, what)
        if name == "mirror" and not orient:  # every sample inside the plane: the reference completes, and says the same
            ref_a, ref_d, rcov = M.describe(planes, octaves, kps, ch, "reference", orient)
            assert rcov.completes.all() and not rcov.next_row.any()
            assert not (cov.left | cov.right | cov.top | cov.bottom).any()
            assert np.array_equal(ref_d, exp_d) and np.array_equal(bits(ref_a), bits(exp_a))
    res.close()
