"""The numpy statement of compute_main_orientation / get_mldb_descriptor (tests/mldb_numpy.py, written from the
reference's text) against the CPU oracle, bit for bit and keypoint for keypoint: a second, independent witness for the
oracle, and the proof that the statement may stand in for the reference where the oracle cannot be asked (keypoints
at the border: tests/test_gpu_describe.py).  No GPU."""
import numpy as np
import pytest

import mldb_numpy as M

FRAMES = [(517, 389, 31), (640, 480, 7)]  # (w, h, synthetic frame index); the first is odd-sized


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pyramids(amd, ref):
    """per frame and channel count: (oracle result, planes[level] = (Lt, Lx, Ly), octaves[level])"""
    out = {}
    for w, h, idx in FRAMES:
        frame = amd.synth_frame(w, h, idx)
        for ch in (3, 1, 2):
            rf = ref.extract(frame, ref.default_config(descriptor_channels=ch))
            planes = [tuple(rf.plane(l, p) for p in ("Lt", "Lx", "Ly")) for l in range(rf.num_levels)]
            octaves = [rf.level_info(l)["octave"] for l in range(rf.num_levels)]
            out[(w, h, ch)] = (rf, planes, octaves)
    return out


def check_against_oracle(rf, planes, octaves, kps, ch, orient):
    """statement == oracle on keypoints whose samples all lie inside their plane (the oracle's reads are unchecked: the
    statement vouches for that first); returns the statement's (angles, descriptors)"""
    a_ref, d_ref, cov = M.describe(planes, octaves, kps, ch, "reference", orient)
    assert cov.completes.all() and not cov.next_row.any()
    a_cl, d_cl, cov_cl = M.describe(planes, octaves, kps, ch, "clamped", orient)
    assert not (cov_cl.left | cov_cl.right | cov_cl.top | cov_cl.bottom).any()
    assert np.array_equal(bits(a_ref), bits(a_cl)) and np.array_equal(d_ref, d_cl)  # interior: the two forms are one
    k_or, d_or = rf.describe(kps, compute_orientation=orient)
    bad_a = np.nonzero(bits(a_ref) != bits(k_or["angle"]))[0]
    bad_d = np.nonzero((d_ref != d_or).any(axis=1))[0]
    assert len(bad_a) == 0 and len(bad_d) == 0, (len(kps), bad_a[:5], bad_d[:5])
    return a_ref, d_ref


@pytest.mark.parametrize("ch", [3, 1, 2])
@pytest.mark.parametrize("w,h,idx", FRAMES)
def test_statement_equals_oracle_on_detected_keypoints(pyramids, w, h, idx, ch):
    rf, planes, octaves = pyramids[(w, h, ch)]
    kp, desc = rf.keypoints(), rf.descriptors()
    assert len(kp) > 50 and desc.shape[1] == (162 * ch + 7) // 8
    assert len(np.unique(kp["class_id"])) >= 3
    for sampling in ("reference", "clamped"):
        ang, d, cov = M.describe(planes, octaves, kp, ch, sampling)
        assert np.array_equal(bits(ang), bits(kp["angle"])), sampling     # every keypoint, every bit
        assert np.array_equal(d, desc), sampling
        assert cov.completes.all() and not cov.next_row.any()
        assert not (cov.left | cov.right | cov.top | cov.bottom).any()
    # with the stored angle instead of a recomputed one
    _, d, _ = M.describe(planes, octaves, kp, ch, "reference", compute_orientation=False)
    assert np.array_equal(d, desc)


@pytest.mark.parametrize("ch", [3, 1, 2])
@pytest.mark.parametrize("w,h,idx", FRAMES)
def test_statement_equals_oracle_on_moved_keypoints(pyramids, w, h, idx, ch):
    """the detector's keypoints moved, rescaled and re-angled: still inside (the detector keeps twice the lattice's reach
    from the border), but no longer what the detector emitted"""
    rf, planes, octaves = pyramids[(w, h, ch)]
    kp = rf.keypoints()
    n = len(kp)
    variants = []
    for dx, dy, sz in ((1.3, -0.7, 1.1), (-2.5, 0.5, 0.8), (0.0, 0.0, 1.3)):
        k = kp.copy()
        k["x"] += np.float32(dx)
        k["y"] += np.float32(dy)
        k["size"] *= np.float32(sz)
        k["angle"] = np.linspace(-np.pi, np.pi, n).astype(np.float32)
        variants.append(k)
    k = kp.copy()  # the angles where the descriptor kernel's lattice walk changes direction, and far outside [-pi, pi]
    special = np.array([0.0, -0.0, np.pi / 4, -np.pi / 4, 3 * np.pi / 4, -3 * np.pi / 4, np.pi / 2, -np.pi / 2, np.pi, -np.pi,
                        1000.0], np.float32)
    k["angle"] = special[np.arange(n) % len(special)]
    variants.append(k)
    moved = np.concatenate(variants)
    for orient in (True, False):
        ang, _ = check_against_oracle(rf, planes, octaves, moved, ch, orient)
        if not orient:
            assert np.array_equal(bits(ang), bits(moved["angle"]))


@pytest.mark.parametrize("ch", [3, 2])
@pytest.mark.parametrize("w,h,idx", FRAMES)
def test_orientation_uses_the_levels_octave_and_the_descriptor_the_keypoints(pyramids, w, h, idx, ch):
    """scale_space_extrema.rs:279 takes the ratio from evolutions[class_id].octave, descriptors.rs:51 from keypoint.octave.
    Keypoints built so that both ops stay inside the plane with the keypoint's octave one above / one below its level's."""
    rf, planes, octaves = pyramids[(w, h, ch)]
    rows = []
    for lvl, o in enumerate(octaves):
        lh, lw = planes[lvl][0].shape
        for delta in (1, -1):
            if o + delta < 0:
                continue
            # descriptor: centre (px, py), scale 1, reach 10.5 * sqrt(2) < 15; orientation: centre (px, py) * 2^delta, scale round(2^delta), reach 6 scales
            hi_x, hi_y = ((lw - 14) // 2, (lh - 14) // 2) if delta > 0 else (lw - 18, lh - 18)
            assert hi_x >= 16 and hi_y >= 16, (lvl, lw, lh)
            for px in np.linspace(16, hi_x, 7):
                for py in np.linspace(16, hi_y, 5):
                    r = 2.0 ** (o + delta)
                    rows.append((np.float32(px) * r, np.float32(py + 0.5) * r, 0.0, 2.0 * r, o + delta, lvl, 0.6, 0))
    kps = np.array(rows, M.KEYPOINT_DTYPE)
    assert len(kps) > 300
    ang, desc = check_against_oracle(rf, planes, octaves, kps, ch, True)
    same = kps.copy()
    same["octave"] = np.array(octaves, np.uint64)[kps["class_id"]]
    # (the orientation of `same` samples where that of `kps` does; its descriptor lattice may leave the plane, so the
    # statement alone is asked, in its clamped form)
    ang_same, desc_same, _ = M.describe(planes, octaves, same, ch, "clamped", True)
    assert np.array_equal(bits(ang), bits(ang_same))                 # the orientation does not look at keypoint.octave
    assert (desc != desc_same).any(axis=1).sum() > len(kps) * 0.9    # the descriptor does
    assert len(np.unique(bits(ang))) > len(kps) // 2                 # (and the angles are the planes', not the given 0.6)


def test_round_is_half_away_from_zero():
    x = np.array([0.5, -0.5, 1.5, 2.5, -2.5, 0.49999997, -0.49999997, 8388609.0, -8388609.0, 0.0, -0.0, np.inf, -np.inf, 1e30],
                 np.float32)
    want = np.array([1, -1, 2, 3, -3, 0, -0.0, 8388609.0, -8388609.0, 0.0, -0.0, np.inf, -np.inf, 1e30], np.float32)
    assert np.array_equal(bits(M.round_f32(x)), bits(want))
    assert np.isnan(M.round_f32(np.array([np.nan], np.float32))[0])


def test_sampling_forms_at_the_border():
    """a 6 x 4 plane whose value is its flat index: what each form reads, and what it reports"""
    w, h = 6, 4
    fx = np.array([2, 7, 7, -1, np.nan, 1e30, 5], np.float32)
    fy = np.array([1, 1, 3, 2, 2, 0, np.inf], np.float32)
    cov = M.Coverage(len(fx))
    got = M._Sampler(w, h, "reference", cov).index(fx, fy, orientation=False)
    #            in-plane, next row, past the buffer, negative, NaN -> 0, far out, far out
    assert cov.completes.tolist() == [True, True, False, False, True, False, False]
    assert cov.next_row.tolist() == [False, True, False, False, False, False, False]
    assert got[[0, 1, 4]].tolist() == [8, 13, 12]
    cov = M.Coverage(len(fx))
    got = M._Sampler(w, h, "reference", cov).index(fx, fy, orientation=True)   # `as usize`: the negative becomes 0
    assert cov.completes.tolist() == [True, True, False, True, True, False, False] and got[3] == 12
    cov = M.Coverage(len(fx))
    got = M._Sampler(w, h, "clamped", cov).index(fx, fy, orientation=False)
    assert got.tolist() == [8, 11, 23, 12, 12, 5, 23]
    assert cov.right.tolist() == [False, True, True, False, False, True, False]
    assert cov.left.tolist() == [False, False, False, True, False, False, False]
    assert cov.bottom.tolist() == [False, False, False, False, False, False, True] and not cov.top.any()
