"""Keypoint detection -- find_scale_space_extrema + do_subpixel_refinement (scale_space_extrema.rs:12-189) -- on the CPU:
the numpy statement (tests/extrema_numpy.py) is pinned to the oracle on natural frames; the oracle and the product's host
selection (akz_host_select_keypoints) are held to the statement on the crafted pyramids (tests/extrema_cases.py); and the
crafted pyramids are shown to have teeth: every mutation switch of the statement changes the keypoints of the cases named in
CATCHES, and every case changes under at least one switch.  Everything is compared for equality; no GPU call."""
import functools

import numpy as np
import pytest

import extrema_cases as X
import extrema_numpy as E

FIELDS = ("x", "y", "response", "size", "octave", "class_id")

# what the statement gives per case: (extrema before the refinement, keypoints) -- the cases' docstrings say why
EXPECTED = {"strict": (4, 4), "border": (16, 16), "dist_same_level": (6, 6), "dist_same_level_size3": (6, 6), "dist_prev_level": (4, 4),
            "dist_prev_level_octave": (3, 3), "dist_next_level": (3, 3), "dist_default": (3, 3), "response": (8, 8),
            "order_first_hit": (7, 7), "order_second_pass_earlier": (2, 2), "order_second_pass_later": (1, 1), "gate": (20, 10)}
EXPECTED = {k: (e + X.FILL, n + X.FILL) for k, (e, n) in EXPECTED.items()}  # ... and the fillers, each a keypoint

# per switch, the cases (by prefix) that MUST give other keypoints under it; test_teeth prints the whole matrix
CATCHES = {
    "nms_ge": ("strict",),
    "thr_ge": ("strict", "dist_default"),
    "dist_lt": ("dist_same_level", "dist_same_level_size3", "dist_prev_level", "dist_prev_level_octave", "dist_next_level",
                "order_second_pass_later"),
    "resp_ge": ("response",),
    "gate_lt": ("gate",),
    "any_hit_not_first": ("order_first_hit", "order_second_pass_earlier", "dense"),
    "second_pass_any_position": ("order_second_pass_earlier",),
    "prev_level_at_level0": ("dist_prev_level",),
    "border_lo_le": ("border",),
    "border_hi_gt": ("border",),
}


def prefix(name):
    return name.rsplit("_", 1)[0]


@functools.lru_cache(maxsize=None)
def built(name):
    return X.pyramid(X.CASE_FN[name]())


@functools.lru_cache(maxsize=None)
def stated(name, mut=()):
    _, _, cfg, levels, ldets = built(name)
    return E.detect(ldets, levels, cfg, mut)


def same_keypoints(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in FIELDS)


def assert_keypoints(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for f in FIELDS:
        ga, ea = np.asarray(got[f]), np.asarray(exp[f])
        if ga.dtype.kind == "f":
            ga, ea = ga.view(np.uint32), ea.view(np.uint32)
        assert np.array_equal(ga, ea), (what, f, np.nonzero(ga != ea)[0][:5])


def test_statement_plans_like_the_library(amd):
    """the defaults and the level plan the crafted cases assume are the library's"""
    d = amd.Config()
    for k, v in X.DEFAULTS.items():
        assert getattr(d, k) == v, k
    for name in X.CASE_NAMES:
        w, h, cfg, levels, _ = built(name)
        over = {k: getattr(cfg, k) for k in X.DEFAULTS}
        plan = amd.plan_levels(w, h, amd.Config(**over))
        assert [(p["w"], p["h"], p["octave"], p["esigma"]) for p in plan] == levels, name


@pytest.mark.parametrize("w,h,idx,kw", [(320, 240, 0, {}), (517, 389, 2, {}),
                                        (320, 240, 1, dict(num_sublevels=3, derivative_factor=1.7, detector_threshold=0.0001)),
                                        (517, 389, 3, dict(num_sublevels=3, max_octave_evolution=3, base_scale_offset=1.3, detector_threshold=0.0002))])
def test_statement_matches_oracle_on_natural_frames(amd, ref, w, h, idx, kw):
    """The statement on the oracle's own Ldet planes gives ref.extract's keypoints: number, order and every field but the
    angle bit for bit, and the extrema count.  This pins the statement."""
    frame = amd.synth_frame(w, h, idx)
    cfg = ref.default_config(**kw)
    rf = ref.extract(frame, cfg)
    infos = [rf.level_info(l) for l in range(rf.num_levels)]
    levels = [(i["w"], i["h"], i["octave"], i["esigma"]) for i in infos]
    assert levels == E.plan_levels(w, h, cfg.num_sublevels, cfg.max_octave_evolution, cfg.base_scale_offset)
    ldets = [rf.plane(l, "Ldet") for l in range(rf.num_levels)]
    kps, n_ext = E.detect(ldets, levels, cfg)
    print(f"{w}x{h} {kw}: {n_ext} extrema, {len(kps)} keypoints")
    assert rf.num_keypoints >= 15 and n_ext == rf.num_extrema
    assert_keypoints(kps, rf.keypoints(), (w, h, kw))
    rf.close()


def admitted_candidates(name):
    """candidates that pass the border test: what k_nms emits.  More than 16, the smallest candidate list, in every case:
    tests/test_gpu_crafted_extrema.py relies on it for the overflow retry"""
    _, _, cfg, levels, ldets = built(name)
    n = 0
    for lv, d in zip(levels, ldets):
        idx = E.candidates(d, np.float32(cfg.detector_threshold))
        n += int((~E.is_out(idx % lv[0], idx // lv[0], lv, cfg)).sum())
    return n


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_cases_give_what_they_say(name):
    if prefix(name) == "dense":
        kps, n_ext = stated(name)
        assert 20 < len(kps) == n_ext < 720 == admitted_candidates(name)
        return
    kps, n_ext = stated(name)
    assert (n_ext, len(kps)) == EXPECTED[prefix(name)], (name, n_ext, len(kps))
    assert admitted_candidates(name) > 16, name  # (with the fillers; the dense case by itself)


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_oracle_on_crafted_pyramids(ref, name):
    """the oracle's detect on caller-supplied planes (ref_detect_from_planes) against the statement; its angles and descriptor
    rows against the numpy statement of those two ops (tests/mldb_numpy.py) on the same random Lt / Lx / Ly"""
    import mldb_numpy as M
    w, h, cfg, levels, ldets = built(name)
    aux = X.aux_planes(levels, 11)
    planes = [dict(aux[l], Ldet=ldets[l]) for l in range(len(levels))]
    rcfg = ref.default_config(**{k: getattr(cfg, k) for k in X.DEFAULTS})
    rf = ref.detect_from_planes(w, h, planes, rcfg)
    kps, n_ext = stated(name)
    assert rf.num_extrema == n_ext
    got = rf.keypoints()
    assert_keypoints(got, kps, name)
    ang, desc, cov = M.describe([(a["Lt"], a["Lx"], a["Ly"]) for a in aux], [lv[2] for lv in levels], got, 3, "reference")
    assert cov.completes.all()
    assert np.array_equal(got["angle"].view(np.uint32), ang.view(np.uint32)) and np.array_equal(rf.descriptors(), desc), name
    rf.close()


def candidate_records(amd, name):
    """the statement's candidates that pass the border test, as akz_host_select_keypoints takes them, in scan order"""
    _, _, cfg, levels, ldets = built(name)
    out = []
    for l, lv in enumerate(levels):
        d = ldets[l]
        idx = E.candidates(d, np.float32(cfg.detector_threshold))
        xs, ys = idx % lv[0], idx // lv[0]
        ok = ~E.is_out(xs, ys, lv, cfg)
        for i, x, y in zip(idx[ok], xs[ok], ys[ok]):
            out.append((l, i, d[y, x], d[y, x + 1], d[y, x - 1], d[y + 1, x], d[y - 1, x], 0))
    return np.array(out, amd.CANDIDATE_DTYPE)


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_host_selection_on_crafted_pyramids(amd, name):
    """akz_host_select_keypoints (the grid selection of akz_keypoints.cpp) on the statement's candidates, in scan order and
    in a random permutation"""
    w, h, cfg, _, _ = built(name)
    acfg = amd.Config(**{k: getattr(cfg, k) for k in X.DEFAULTS})
    cands = candidate_records(amd, name)
    kps, n_ext = stated(name)
    rng = np.random.default_rng(5)
    for order in (np.arange(len(cands)), rng.permutation(len(cands))):
        got, got_ext = amd.host_select_keypoints(w, h, acfg, cands[order])
        assert got_ext == n_ext, name
        assert_keypoints(got, kps, name)


def test_teeth():
    """Every switch changes the keypoint list of the cases CATCHES names for it, no switch is left uncaught, and no case is
    decoration: each one changes under at least one switch.  Statement against statement: the code under test has no say."""
    matrix = {s: [n for n in X.CASE_NAMES if not same_keypoints(stated(n, (s,))[0], stated(n)[0])] for s in E.SWITCHES}
    for s in E.SWITCHES:
        print(f"{s:26s} caught by {matrix[s]}")
    assert set(CATCHES) == set(E.SWITCHES)
    for s, must in CATCHES.items():
        for n in X.CASE_NAMES:
            if prefix(n) in must:
                assert n in matrix[s], (s, n)
        assert matrix[s], s
    caught = {n for v in matrix.values() for n in v}
    for n in X.CASE_NAMES:
        assert n in caught, n
