"""Guided matching on the host (akz_descriptor_match_guided_host, no GPU): the list against a numpy statement of the gate
and the scan written here, the tie to the oracle's blind descriptor_match when the gate passes everything, degenerate
models, and every refusal of the host and the context calls (which all come before any GPU work)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from match_numpy import scan_admitted
from test_match_pairs_host import _status

F32 = np.float32
NEW_SYMBOLS = ("akz_descriptor_match_guided_host", "akz_descriptor_match_guided", "akz_descriptor_match_guided_pairs",
               "akz_match_features_homography_guided", "akz_match_features_homography_guided_pairs")


def test_symbols(amd):
    L = amd.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
    assert L.akz_abi_version() == 6
    assert (amd.GUIDED_HOMOGRAPHY, amd.GUIDED_FUNDAMENTAL) == (0, 1)


# ---- the numpy statement ---------------------------------------------------------------------------------------------------
def np_gate(kind, model, x0, y0, x1, y1, radius):
    """The gate of one query (x0, y0: np.float32 scalars) on all train points (x1, y1: float32 arrays), every operation in
    f32 in the order the header states; numpy rounds each one and never fuses."""
    m = np.asarray(model, F32).reshape(9)
    r = F32(radius)
    with np.errstate(all="ignore"):
        if kind == 0:
            w = (m[6] * x0 + m[7] * y0) + m[8]
            u = (m[0] * x0 + m[1] * y0) + m[2]
            v = (m[3] * x0 + m[4] * y0) + m[5]
            du = u - x1 * w
            dv = v - y1 * w
            ew = r * w
            return (w > F32(0)) & (du * du + dv * dv < ew * ew)
        l0 = (m[0] * x0 + m[1] * y0) + m[2]
        l1 = (m[3] * x0 + m[4] * y0) + m[5]
        l2 = (m[6] * x0 + m[7] * y0) + m[8]
        n = l0 * l0 + l1 * l1
        r2 = r * r
        s = (l0 * x1 + l1 * y1) + l2
        return s * s < r2 * n


def np_guided(k0, d0, k1, d1, model, kind, radius, threshold, ratio):
    """feature_matching.rs:37-81 with `if !gate { continue }` at the top of the inner loop: the gate is stated here, the scan over
    the rows it admits is the one of tests/match_numpy.py."""
    n0, n1 = len(d0), len(d1)
    x1, y1 = k1["x"][:n1].astype(F32), k1["y"][:n1].astype(F32)
    ok = np.zeros((n0, n1), bool)
    for i in range(n0 if n1 else 0):
        ok[i] = np_gate(kind, model, F32(k0["x"][i]), F32(k0["y"][i]), x1, y1, radius)
    return _as_list(scan_admitted(d0, d1, ok, threshold, ratio))


def _as_list(m):
    return [(int(a), int(b), float(c)) for a, b, c in zip(m["index_0"], m["index_1"], m["distance"])]


H_MODEL = np.array([[0.98, -0.05, 12.0], [0.04, 1.01, -7.0], [1e-5, -2e-5, 1.0]])


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


F_MODEL = _skew((1.0, 0.5, 0.001))  # a pure translation of a pinhole camera (K = I): epipole at (1000, 500), outside the points


def _case(amd, nb, seed, n0=90, n1=130):
    """Random sets; a third of the train points are planted near H_MODEL p0 (0.2 .. 4 px away, so that radii 0.5 and 3 pass
    some), a third of the train DESCRIPTORS are near copies of query rows.  Duplicates: rows 0..9 of the train set are
    exact copies of rows 100..109 (descriptor AND keypoint: a tie that the lowest index wins), rows 10..19 carry the
    descriptors of rows 110..119 but lie 200 px away (gated out for small radii: then the HIGHER index must win)."""
    rng = np.random.default_rng(seed)
    k0 = np.zeros(n0 + 7, amd.KEYPOINT_DTYPE)  # more keypoints than descriptors
    k1 = np.zeros(n1 + 3, amd.KEYPOINT_DTYPE)
    for k in (k0, k1):
        k["x"] = rng.uniform(0, 500, len(k))
        k["y"] = rng.uniform(0, 300, len(k))
    d0 = rng.integers(0, 256, (n0, nb), dtype=np.uint8)
    d1 = rng.integers(0, 256, (n1, nb), dtype=np.uint8)
    src = rng.permutation(n0)[: n1 // 3]
    p = np.c_[k0["x"][src], k0["y"][src], np.ones(len(src))].astype(np.float64) @ H_MODEL.T
    ang, rad = rng.uniform(0, 2 * np.pi, len(src)), rng.uniform(0.2, 4.0, len(src))
    at = 20 + np.arange(len(src))
    k1["x"][at] = p[:, 0] / p[:, 2] + rad * np.cos(ang)
    k1["y"][at] = p[:, 1] / p[:, 2] + rad * np.sin(ang)
    noisy = d0[src].copy()
    flip = rng.integers(0, nb, (len(src), 3))
    for r in range(len(src)):
        noisy[r, flip[r]] ^= rng.integers(1, 256, 3).astype(np.uint8)
    d1[at] = noisy
    d1[100:120], k1[100:120] = d1[20:40], k1[20:40]  # (moved: rows 20..39 become random again)
    d1[20:40] = rng.integers(0, 256, (20, nb), dtype=np.uint8)
    k1["x"][20:40], k1["y"][20:40] = rng.uniform(0, 500, 20), rng.uniform(0, 300, 20)
    d1[0:10], k1[0:10] = d1[100:110], k1[100:110]
    d1[10:20] = d1[110:120]
    k1["x"][10:20] = k1["x"][110:120] + 200.0
    k1["y"][10:20] = k1["y"][110:120]
    return k0, d0, k1, d1


@pytest.mark.parametrize("nb", [21, 41, 61, 64])
def test_host_equals_numpy(amd, nb):
    k0, d0, k1, d1 = _case(amd, nb, seed=nb)
    small = 8 * nb // 3  # below most random distances (mean 4 nb), above the planted ones
    nonempty = ties_low = ties_high = 0
    for (kind, model), radius, thr, ratio in itertools.product(((0, H_MODEL), (1, F_MODEL)), (0.0, 0.5, 3.0, 50.0),
                                                               (10000, small), (0.6, 0.86, 1.0)):
        got = _as_list(amd.descriptor_match_guided_host(k0, d0, k1, d1, model, kind, radius, thr, ratio))
        exp = np_guided(k0, d0, k1, d1, model, kind, radius, thr, ratio)
        assert got == exp, (nb, kind, radius, thr, ratio, len(got), len(exp))
        nonempty += bool(exp)
        if radius == 0.0:
            assert exp == []
    # the duplicates decide: with the twin in the gate the lower index is reported, with the twin 200 px away the higher
    # (a ratio above 1, since a query whose two best are equal fails min < second ratio^2 at any ratio up to 1)
    wide = _as_list(amd.descriptor_match_guided_host(k0, d0, k1, d1, H_MODEL, 0, 1e4, 10000, 1.5))
    near = _as_list(amd.descriptor_match_guided_host(k0, d0, k1, d1, H_MODEL, 0, 3.0, 10000, 1.5))
    assert near == np_guided(k0, d0, k1, d1, H_MODEL, 0, 3.0, 10000, 1.5)
    assert wide == np_guided(k0, d0, k1, d1, H_MODEL, 0, 1e4, 10000, 1.5)
    ties_low = sum(j < 10 for _, j, _ in near)
    ties_high = sum(110 <= j < 120 for _, j, _ in near)
    assert nonempty >= 24 and ties_low > 0 and ties_high > 0, (nonempty, ties_low, ties_high)
    assert not any(110 <= j < 120 for _, j, _ in wide)  # ungated, rows 10..19 win those ties


@pytest.mark.parametrize("nb", [21, 61, 64])
def test_all_pass_gate_equals_the_oracle(amd, ref, nb):
    """A gate that passes every pair leaves the blind scan.  Why it passes, for points in [0, 500] x [0, 300]:
    H = I, radius 1e18: w = 1 exactly, ew = 1e18, ew ew = 1e36 is finite in f32 (max 3.4e38) and du du + dv dv <= 500^2 +
    300^2 < 1e36.  F = [t]x with t = (1, 0.5, 0.001): the epipole (1000, 500) lies outside the points, so l0 = 0.5 - 0.001 y0
    >= 0.2 and n >= 0.04: r2 n >= 4e34 (or +inf when it overflows, which compares the same way), while |s| <= |l0| 500 +
    |l1| 300 + |l2| < 1e3, s s < 1e6."""
    k0, d0, k1, d1 = _case(amd, nb, seed=100 + nb)
    for ratio, thr in ((0.86, 10000), (0.6, 10000), (1.0, 8 * nb // 3)):
        exp = ref.descriptor_match(d0, d1, thr, ratio)
        assert len(exp) > 0 or ratio == 0.6
        for kind, model in ((0, np.eye(3)), (1, F_MODEL)):
            got = amd.descriptor_match_guided_host(k0, d0, k1, d1, model, kind, 1e18, thr, ratio)
            assert got.dtype == exp.dtype and np.array_equal(got, exp), (nb, kind, ratio, thr)


def test_degenerate_models_pass_nothing(amd):
    k0, d0, k1, d1 = _case(amd, 61, seed=3)
    nan_h, nan_f = H_MODEL.copy(), F_MODEL.copy()
    nan_h[2, 2] = np.nan
    nan_f[0, 1] = np.nan
    cases = [(1, np.zeros((3, 3)), 3.0), (0, nan_h, 50.0), (1, nan_f, 50.0), (0, np.full((3, 3), np.nan), 1e18),
             (0, H_MODEL, 0.0), (1, F_MODEL, 0.0), (0, np.eye(3), 0.0)]
    for kind, model, radius in cases:
        got = amd.descriptor_match_guided_host(k0, d0, k1, d1, model, kind, radius, 10000, 1.0)
        assert len(got) == 0, (kind, radius)
    # empty sets are fine
    e_k, e_d = np.zeros(0, amd.KEYPOINT_DTYPE), np.zeros((0, 61), np.uint8)
    assert len(amd.descriptor_match_guided_host(e_k, e_d, k1, d1, H_MODEL, 0, 3.0)) == 0
    assert len(amd.descriptor_match_guided_host(k0, d0, e_k, e_d, H_MODEL, 0, 3.0)) == 0


def test_refusals(amd):
    """Every refusal is AKZ_ERR_INVALID_ARG with a message and leaves out / n_out as they were; those of the context
    calls come before any GPU work (they are made here with a NULL context, on a machine without a GPU)."""
    L = amd.lib()
    bad = _status(amd)
    k0, d0, k1, d1 = _case(amd, 61, seed=9)
    model = np.ascontiguousarray(H_MODEL.reshape(9), F32)
    vp, fp = C.c_void_p, C.POINTER(C.c_float)

    def pair_call(fn, first, untouched=True, **kw):
        a = dict(kp0=k0.ctypes.data_as(vp), n_kp0=len(k0), d0=d0.ctypes.data_as(vp), n_d0=len(d0), kp1=k1.ctypes.data_as(vp),
                 n_kp1=len(k1), d1=d1.ctypes.data_as(vp), n_d1=len(d1), nb=61, kind=0, model=model.ctypes.data_as(fp),
                 radius=3.0, out=True, n_out=True)
        a.update(kw)
        o = np.full(len(d0) * 24, 0xAB, np.uint8)
        n = np.full(1, 7, np.uint64)
        st = fn(*first, a["kp0"], a["n_kp0"], a["d0"], a["n_d0"], a["kp1"], a["n_kp1"], a["d1"], a["n_d1"], a["nb"], a["kind"],
                a["model"], a["radius"], 10000, 0.86, o.ctypes.data_as(vp) if a["out"] else None,
                n.ctypes.data_as(C.POINTER(C.c_uint64)) if a["n_out"] else None)
        assert not untouched or (np.all(o == 0xAB) and n[0] == 7)
        return st, L.akz_last_error().decode()

    refusals = [(dict(n_kp0=len(d0) - 1), "more descriptors"), (dict(n_kp1=len(d1) - 1), "more descriptors"),
                (dict(nb=0), "desc_bytes"), (dict(nb=65), "desc_bytes"), (dict(kp0=None), "null"), (dict(d0=None), "null"),
                (dict(kp1=None), "null"), (dict(d1=None), "null"), (dict(out=False), "out"), (dict(n_out=False), "n_out"),
                (dict(model=None), "model"), (dict(kind=-1), "model_kind"), (dict(kind=2), "model_kind"),
                (dict(radius=-1.0), "radius"), (dict(radius=float("nan")), "radius"), (dict(radius=float("inf")), "radius")]
    for fn, first in ((L.akz_descriptor_match_guided_host, ()), (L.akz_descriptor_match_guided, (None,))):
        for kw, word in refusals:
            st, msg = pair_call(fn, first, **kw)
            assert st == bad and word in msg, (fn.__name__, kw, msg)
    st, msg = pair_call(L.akz_descriptor_match_guided, (None,))  # nothing wrong but the context
    assert st == bad and "context" in msg
    st, _ = pair_call(L.akz_descriptor_match_guided_host, (), untouched=False)  # and the host call needs none
    assert st == 0

    # the pairs call and the composite
    sets = (amd.FeatureSet * 2)(amd.FeatureSet(k0.ctypes.data_as(vp), len(k0), d0.ctypes.data_as(vp), len(d0)),
                                amd.FeatureSet(k1.ctypes.data_as(vp), len(k1), d1.ctypes.data_as(vp), len(d1)))
    short = (amd.FeatureSet * 2)(sets[0], amd.FeatureSet(k1.ctypes.data_as(vp), 5, d1.ctypes.data_as(vp), len(d1)))
    models = np.ascontiguousarray(np.tile(model, 2))

    def pairs_call(composite, s=sets, pairs=((0, 1), (1, 0)), nb=61, kind=0, mdl=True, radius=3.0, out=True):
        pr = np.asarray(pairs, np.uint64).reshape(-1)
        o = np.full(1 << 14, 0xAB, np.uint8)
        n = np.full(2, 7, np.uint64)
        h = np.full(18, 5.0, F32)
        f = np.full(2, 9, np.int32)
        head = (None, C.cast(s, vp), 2, pr.ctypes.data_as(vp), len(pr) // 2, nb)
        tail = (o.ctypes.data_as(vp) if out else None, n.ctypes.data_as(C.POINTER(C.c_uint64)))
        if composite:
            st = L.akz_match_features_homography_guided_pairs(*head, 0.86, 100, 3.0, radius, 0.86, *tail, h.ctypes.data_as(fp),
                                                              f.ctypes.data_as(C.POINTER(C.c_int32)))
        else:
            st = L.akz_descriptor_match_guided_pairs(*head, kind, models.ctypes.data_as(fp) if mdl else None, radius, 10000, 0.86,
                                                     *tail)
        assert np.all(o == 0xAB) and np.all(n == 7) and np.all(h == 5.0) and np.all(f == 9)
        return st, L.akz_last_error().decode()

    assert L.akz_descriptor_match_guided_pairs(None, None, 0, None, 0, 61, 0, None, 3.0, 10000, 0.86, None, None) == 0
    assert L.akz_match_features_homography_guided_pairs(None, None, 0, None, 0, 61, 0.86, 10, 3.0, 3.0, 0.86, None, None, None,
                                                        None) == 0
    for composite in (False, True):
        for kw, word in ((dict(), "context"), (dict(s=short), "more descriptors"), (dict(nb=65), "desc_bytes"),
                         (dict(pairs=((0, 1), (1, 2))), "set index 2"), (dict(out=False), "out"),
                         (dict(radius=-0.5), "radius"), (dict(radius=float("nan")), "radius")):
            st, msg = pairs_call(composite, **kw)
            assert st == bad and word in msg, (composite, kw, msg)
    for kw, word in ((dict(kind=3), "model_kind"), (dict(mdl=False), "model")):
        st, msg = pairs_call(False, **kw)
        assert st == bad and word in msg, (kw, msg)
    # the one-pair composite
    o = np.full(len(d0) * 24, 0xAB, np.uint8)
    n = np.full(1, 7, np.uint64)
    for n_kp0, radius, word in ((len(d0) - 1, 3.0, "more descriptors"), (len(k0), -1.0, "radius"), (len(k0), 3.0, "context")):
        st = L.akz_match_features_homography_guided(None, k0.ctypes.data_as(vp), n_kp0, d0.ctypes.data_as(vp), len(d0),
                                                    k1.ctypes.data_as(vp), len(k1), d1.ctypes.data_as(vp), len(d1), 61, 0.86, 100, 3.0,
                                                    radius, 0.86, o.ctypes.data_as(vp), n.ctypes.data_as(C.POINTER(C.c_uint64)), None, None)
        assert st == bad and word in L.akz_last_error().decode() and np.all(o == 0xAB) and n[0] == 7
    st = L.akz_match_features_homography_guided(None, k0.ctypes.data_as(vp), len(k0), d0.ctypes.data_as(vp), len(d0),
                                                k1.ctypes.data_as(vp), len(k1), d1.ctypes.data_as(vp), len(d1), 61, 0.86, 100, 3.0, 3.0,
                                                0.86, o.ctypes.data_as(vp), None, None, None)
    assert st == bad and "n_out" in L.akz_last_error().decode() and np.all(o == 0xAB)
