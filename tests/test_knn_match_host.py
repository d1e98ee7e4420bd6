"""k-nearest-neighbour matching on the host (akz_descriptor_match_knn_host; no GPU call): the whole buffers -- records, padding
slots and counts -- against the independent numpy statement of tests/match_numpy.py (distances from np.unpackbits; a stable argsort
per row, which orders by (distance, index); a cut at the threshold and at k), the tie rule on a train set of repeated rows, the
refusals, the two empty cases and the declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from match_numpy import NO_ROW, distances, knn
from test_match_pairs_host import ROOT

NEW_SYMBOLS = ("akz_descriptor_match_knn_host", "akz_descriptor_match_knn", "akz_descriptor_match_knn_device")
KS = (1, 2, 3, 5, 8)


def numpy_knn(amd, a, b, k, thr, dist=None):
    """the statement of include/akaze_hip.h in numpy (tests/match_numpy.py) -> (records (n0, k), counts (n0,))"""
    out, counts = knn(a, b, k, thr, dist)
    assert out.dtype == amd.MATCH_DTYPE
    return out, counts


def same(got, exp, what):
    (g_out, g_cnt), (e_out, e_cnt) = got, exp
    assert g_out.dtype == e_out.dtype and g_out.shape == e_out.shape and g_cnt.dtype == np.uint32, what
    assert np.array_equal(g_cnt, e_cnt), (what, "counts")
    assert g_out.tobytes() == e_out.tobytes(), (what, "records")        # whole buffers: padding slots and +inf bit for bit


def tie_sets(nb=61, repeats=40, seed=5):
    """train rows: 5 distinct descriptors, each `repeats` times, interleaved (row j is descriptor j % 5); queries: the five
    descriptors with 0, 2, 4, 6, 8 flipped bits -- query i is nearest to descriptor i, at the same distance for all its copies"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (5, nb), dtype=np.uint8)
    b = base[np.arange(5 * repeats) % 5]
    a = base.copy()
    for i in range(5):
        for bit in rng.permutation(8 * nb)[:2 * i]:
            a[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    return a, b


def test_symbols_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "akaze_hip_debug.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert hasattr(L, "akz_debug_set_knn_chunks") and "akz_debug_set_knn_chunks" in L._declared
    assert re.search(r"\bint\s+akz_debug_set_knn_chunks\s*\(", dbg) and "akz_debug_set_knn_chunks" not in hdr
    assert re.search(r"#define\s+AKZ_KNN_MAX_K\s+8\b", hdr)
    assert L.akz_abi_version() == 6
    assert callable(amd.descriptor_match_knn_host)
    for name in ("descriptor_match_knn", "descriptor_match_knn_device", "set_knn_chunks"):
        assert callable(getattr(amd.Context, name)), name


@pytest.mark.parametrize("nb", [1, 7, 61, 64])
def test_statement_against_numpy(amd, nb):
    rng = np.random.default_rng(100 + nb)
    a = rng.integers(0, 256, (9, nb), dtype=np.uint8)
    seen = set()
    for n1 in (0, 1, 3, 7, 200):
        b = rng.integers(0, 256, (n1, nb), dtype=np.uint8)
        if n1 >= 7:
            b[5] = a[2]                                                   # an exact copy: distance 0
        dist = distances(a, b)
        median = int(np.median(dist)) if n1 else 2
        for thr in (0, 1, median, 8 * nb, 10000):
            for k in KS:
                exp = numpy_knn(amd, a, b, k, thr, dist)
                same(amd.descriptor_match_knn_host(a, b, k, thr), exp, (nb, n1, thr, k))
                seen |= set(exp[1].tolist())
                assert np.all(exp[1] <= min(k, n1))
    assert {0, 1, 2, 3, 5, 7, 8} <= seen                                  # empty, partly filled and full lists all occur


def test_ties_go_to_the_lowest_indices(amd):
    a, b = tie_sets()
    dist = distances(a, b)
    for k in KS:
        out, counts = amd.descriptor_match_knn_host(a, b, k)
        same((out, counts), numpy_knn(amd, a, b, k, 10000, dist), k)
        for i in range(5):                                               # the copies of descriptor i, lowest rows first
            assert np.all(counts == k)
            assert out["index_1"][i].tolist() == [i + 5 * r for r in range(k)], (k, i)
            assert np.all(out["distance"][i] == 2 * i)
    # a threshold that admits the copies alone: 40 of them, k = 8 keeps the first eight
    out, counts = amd.descriptor_match_knn_host(a, b, 8, 9)
    assert np.all(counts == 8) and out["index_1"][4].tolist() == [4 + 5 * r for r in range(8)]


def test_refusals_leave_the_outputs_untouched(amd):
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (6, 61), dtype=np.uint8)
    b = rng.integers(0, 256, (11, 61), dtype=np.uint8)
    L = amd.lib()
    out = np.zeros((6, 8), amd.MATCH_DTYPE)
    out["index_0"] = 77
    counts = np.full(6, 4242, np.uint32)
    pa, pb, po, pc = a.ctypes.data, b.ctypes.data, out.ctypes.data, counts.ctypes.data
    big = 0x80000000
    cases = ((pa, 6, pb, 11, 61, 0, 10000, po, pc),          # k == 0
             (pa, 6, pb, 11, 61, 9, 10000, po, pc),          # k > AKZ_KNN_MAX_K
             (pa, 6, pb, 11, 0, 2, 10000, po, pc),           # desc_bytes == 0
             (pa, 6, pb, 11, 65, 2, 10000, po, pc),          # desc_bytes > 64
             (pa, 6, pb, 11, 61, 2, 10000, None, pc),        # null outputs
             (pa, 6, pb, 11, 61, 2, 10000, po, None),
             (None, 6, pb, 11, 61, 2, 10000, po, pc),        # null inputs with rows
             (pa, 6, None, 11, 61, 2, 10000, po, pc),
             (pa, big, pb, 11, 61, 2, 10000, po, pc),        # too many rows
             (pa, 6, pb, big, 61, 2, 10000, po, pc))
    for n, args in enumerate(cases):
        assert L.akz_descriptor_match_knn_host(*args) == -1, n         # AKZ_ERR_INVALID_ARG
        assert np.all(out["index_0"] == 77) and np.all(counts == 4242), n
    # no context: the GPU forms refuse as well
    assert L.akz_descriptor_match_knn(None, pa, 6, pb, 11, 61, 2, 10000, po, pc) != 0
    assert L.akz_descriptor_match_knn_device(None, pa, 6, pb, 11, 2, 10000, po, pc) != 0
    assert np.all(out["index_0"] == 77) and np.all(counts == 4242)


def test_empty_sets(amd):
    rng = np.random.default_rng(10)
    a = rng.integers(0, 256, (6, 61), dtype=np.uint8)
    L = amd.lib()
    out = np.zeros((6, 3), amd.MATCH_DTYPE)
    out["index_0"] = 77
    counts = np.full(6, 4242, np.uint32)
    # n0 == 0: valid, nothing written (the rows of the empty side may be null)
    assert L.akz_descriptor_match_knn_host(None, 0, a.ctypes.data, 6, 61, 3, 10000, out.ctypes.data, counts.ctypes.data) == 0
    assert np.all(out["index_0"] == 77) and np.all(counts == 4242)
    # n1 == 0: every count 0, every slot padding
    assert L.akz_descriptor_match_knn_host(a.ctypes.data, 6, None, 0, 61, 3, 10000, out.ctypes.data, counts.ctypes.data) == 0
    assert np.all(counts == 0) and np.all(out["index_1"] == NO_ROW) and np.all(np.isposinf(out["distance"]))
    assert np.array_equal(out["index_0"], np.repeat(np.arange(6, dtype=np.uint64)[:, None], 3, axis=1))
    got = amd.descriptor_match_knn_host(a[:0], a, 2)
    assert got[0].shape == (0, 2) and got[1].shape == (0,)
