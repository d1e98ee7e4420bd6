"""akz_match_features_pairs without a GPU: the symbol, its refusals (each before any random draw and any GPU work) and the
sample draws it shares with akz_match_features (the plain `%` loop of estimate_fundamental_matrix.rs:117-121)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _status(amd):
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    return int(re.search(r"AKZ_ERR_INVALID_ARG\s*=\s*(-?\d+)", hdr).group(1))


def _color(amd):
    rgb = (C.c_uint8 * 3)()
    assert amd.lib().akz_random_color(rgb) == 0
    return bytes(rgb)


def _set(amd, n_kp, n_desc, nb=61, seed=0):
    rng = np.random.default_rng(seed)
    k = np.zeros(max(n_kp, 1), amd.KEYPOINT_DTYPE)
    k["x"] = rng.uniform(0, 500, len(k))
    k["y"] = rng.uniform(0, 300, len(k))
    d = rng.integers(0, 256, (max(n_desc, 1), nb), dtype=np.uint8)
    return k, d


def test_symbol_exported_and_declared(amd):
    L = amd.lib()
    assert hasattr(L, "akz_match_features_pairs") and "akz_match_features_pairs" in L._declared
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    assert "akz_match_features_pairs(" in hdr and "akz_feature_set" in hdr
    assert C.sizeof(amd.FeatureSet) == 32


def test_refusals_leave_the_source_untouched(amd):
    """Every refusal returns AKZ_ERR_INVALID_ARG with ctx = NULL, names the pair or set, writes nothing, and leaves the
    calling thread's random source where it was (the next colour is the fresh-seed one)."""
    L = amd.lib()
    bad_status = _status(amd)
    amd.random_seed(42, 69)
    fresh = _color(amd)
    good = [_set(amd, 50, 40, seed=i) for i in range(3)]
    keep = []

    def call(sets, pairs, nb=61, out=True, n_out=True, sets_null=False, pairs_null=False):
        arr = (amd.FeatureSet * max(1, len(sets)))()
        for i, (k, nk, d, nd) in enumerate(sets):
            arr[i] = amd.FeatureSet(k, nk, d, nd)
        pr = np.asarray(pairs, np.uint64).reshape(-1)
        keep.append(pr)
        o = np.full(4096, 0xAB, np.uint8)
        n = np.full(max(1, len(pr) // 2), 7, np.uint64)
        amd.random_seed(42, 69)
        st = L.akz_match_features_pairs(None, None if sets_null else C.cast(arr, C.c_void_p), len(sets),
                                        None if pairs_null else pr.ctypes.data_as(C.c_void_p), len(pr) // 2, nb, 0.86, 100,
                                        3.0, o.ctypes.data_as(C.c_void_p) if out else None,
                                        n.ctypes.data_as(C.POINTER(C.c_uint64)) if n_out else None)
        assert np.all(o == 0xAB) and np.all(n == 7)  # nothing written
        assert _color(amd) == fresh                   # no draw
        return st, L.akz_last_error().decode()

    def fs(k, d, nk=None, nd=None):
        return (k.ctypes.data_as(C.c_void_p) if k is not None else None, len(k) if nk is None else nk,
                d.ctypes.data_as(C.c_void_p) if d is not None else None, len(d) if nd is None else nd)

    sets = [fs(k, d) for k, d in good]
    # n_pairs = 0 is AKZ_OK, even without a context
    assert L.akz_match_features_pairs(None, None, 0, None, 0, 61, 0.86, 100, 3.0, None, None) == 0
    # a null context with work to do (and nothing else wrong)
    st, msg = call(sets, [(0, 1), (1, 2)])
    assert st == bad_status and "context" in msg
    # more descriptors than keypoints, in a set used only by the last pair
    k, d = good[2]
    bad = sets[:2] + [fs(k, d, nk=10, nd=40)]
    st, msg = call(bad, [(0, 1), (1, 0), (0, 2)])
    assert st == bad_status and "pair 2" in msg and "set 2" in msg
    st, msg = call(bad, [(0, 1), (2, 1)])
    assert st == bad_status and "pair 1" in msg
    # desc_bytes outside 1..64
    for nb in (0, 65, 1000):
        st, msg = call(sets, [(0, 1)], nb=nb)
        assert st == bad_status and "desc_bytes" in msg
    # a set index >= n_sets, in the last pair
    st, msg = call(sets, [(0, 1), (1, 2), (2, 3)])
    assert st == bad_status and "pair 2" in msg and "set index 3" in msg
    st, msg = call(sets, [(0, 1), (7, 0)])
    assert st == bad_status and "pair 1" in msg
    # null pointers: keypoints / descriptors of a used set, sets, pairs, out, n_out
    st, msg = call(sets[:2] + [fs(None, good[2][1], nk=50)], [(0, 1), (1, 2)])
    assert st == bad_status and "pair 1, set 2" in msg
    st, msg = call(sets[:2] + [fs(good[2][0], None, nd=40)], [(0, 1), (0, 2)])
    assert st == bad_status and "pair 1, set 2" in msg
    st, msg = call(sets, [(0, 1)], sets_null=True)
    assert st == bad_status
    st, msg = call(sets, [(0, 1)], pairs_null=True)
    assert st == bad_status
    st, msg = call(sets, [(0, 1)], out=False)
    assert st == bad_status and "out" in msg
    st, msg = call(sets, [(0, 1)], n_out=False)
    assert st == bad_status
    # an unused bad set is not a refusal reason: only the null context remains
    st, msg = call(sets + [fs(None, None, nk=5, nd=9)], [(0, 1)])
    assert st == bad_status and "context" in msg


def _xorshift(s0, s1):
    M = (1 << 64) - 1
    while True:
        x, y = s0, s1
        s0 = y
        x ^= (x << 23) & M
        x ^= x >> 17
        x ^= y ^ (y >> 26)
        s1 = x
        yield (x + y) & M


def _plain_draws(s0, s1, n, trials):
    src = _xorshift(s0, s1)
    out = []
    for _ in range(trials):
        picked = []
        while len(picked) < 8:
            j = next(src) % n
            if j not in picked:
                picked.append(j)
        out.extend(sorted(picked))
    return np.array(out, np.uint64)


@pytest.mark.parametrize("n", [8, 9, 10, 16, 64, 1024, 1 << 20, 1 << 31, (1 << 31) - 1, (1 << 32) + 1, (1 << 40) + 12345,
                               0xFFFFFFFFFFFFFFC5, 0x9E3779B97F4A7C15, (1 << 63) + 1, (1 << 64) - 1, 3 * (1 << 62) + 7])
def test_sample_draws_equal_the_plain_modulo_loop(amd, n):
    """The draw loop both match_features paths share (exact remainder without a division) gives the indices of the plain
    `source.read() % n` loop, for small, power-of-two, 2^31 - 1 and odd 64-bit match counts."""
    trials = 40 if n < 64 else 300
    for s0, s1 in ((42, 69), (1, 2), (0xDEADBEEFCAFEF00D, 0x0123456789ABCDEF)):
        got = np.zeros(trials * 8, np.uint64)
        assert amd.lib().akz_debug_ransac_samples(s0, s1, n, trials, got.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
        assert np.array_equal(got, _plain_draws(s0, s1, n, trials)), (n, s0, s1)
