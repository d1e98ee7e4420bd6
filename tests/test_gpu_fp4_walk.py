"""The FP4 tile walk (csrc/akz_fp4_scan.hpp) under both of its one-direction clients, on the same inputs at the walk's own edges:
the top-2 scan (k_match_fp4, match mode 3) against the oracle's descriptor_match and the k-list scan (k_knn_fp4) against
akz_descriptor_match_knn_host, for train sets of T - 1 .. 5 T + 1 rows (T = akz_debug_match_tile_rows: a partial tile, a whole
one, a short last step, several steps) cut into 1, 2, 3 and 5 chunks.  Rows come from 8 base descriptors with about 2 % single-bit
flips, so equal distances sit across every half-lane, sub-tile, tile, step and chunk boundary."""
import numpy as np
import pytest

from test_gpu_knn_match import tile_rows
from test_knn_match_host import same

pytestmark = pytest.mark.gpu

N0 = (33, 513)
CHUNKS = (1, 2, 3, 5)
# (ratio, threshold): every list is non-empty and shorter than n0 on every case (asserted below, and chosen on the CPU in
# tests/test_match_statement_host.py: 19 .. 29 of 33 and 362 .. 381 of 513 at (1.5, 10000), 7 .. 19 and 182 .. 210 at (1.5, 2), where
# the threshold cuts the list).  The former (0.99, 12) gave EMPTY lists on all but one case -- in these sets min == second for every
# query --; it stays in ALSO so that nothing this test held before is lost, but nothing is learnt from it.
TOP2 = ((1.5, 10000), (1.5, 2))
ALSO = ((0.99, 12),)


def train_sizes(T):
    return (T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 5 * T + 1)


def sets(n0, n1):
    rng = np.random.default_rng(n0 * 7919 + n1)
    base = rng.integers(0, 256, (8, 61), dtype=np.uint8)
    d0 = base[rng.integers(0, 8, n0)].copy()
    d1 = base[rng.integers(0, 8, n1)].copy()
    d0[rng.random(d0.shape) < 0.02] ^= 0x10
    d1[rng.random(d1.shape) < 0.02] ^= 0x01
    return d0, d1


def expected(amd, ref, n0, n1):
    """inputs and what the two statements say about them (no GPU call)"""
    d0, d1 = sets(n0, n1)
    top2 = {rt: ref.descriptor_match(d0, d1, rt[1], rt[0]) for rt in TOP2 + ALSO}
    for rt in TOP2:
        assert 0 < len(top2[rt]) < n0, (n0, n1, rt)  # the equalities below are not about empty lists, nor about lists of everything
    return d0, d1, top2, {k: amd.descriptor_match_knn_host(d0, d1, k) for k in (8, 1)}


@pytest.fixture(scope="module")
def cases(amd, ref):
    return {(n0, n1): expected(amd, ref, n0, n1) for n0 in N0 for n1 in train_sizes(tile_rows(amd))}


@pytest.mark.parametrize("n0", N0)
@pytest.mark.parametrize("slot", range(7))
def test_both_clients_at_the_walks_edges(ctx, amd, cases, n0, slot):
    n1 = train_sizes(tile_rows(amd))[slot]
    d0, d1, top2, knn = cases[(n0, n1)]
    try:
        ctx.set_match_mode(3)
        for chunks in CHUNKS:
            ctx.debug_set_match_chunks(chunks, 0)
            ctx.set_knn_chunks(chunks)
            for (ratio, thr), exp in top2.items():
                got = ctx.descriptor_match(d0, d1, thr, ratio)
                assert got.dtype == exp.dtype and np.array_equal(got, exp), (n1, chunks, ratio, thr, len(got), len(exp))
            got = {k: ctx.descriptor_match_knn(d0, d1, k) for k in knn}
            for k, exp in knn.items():
                same(got[k], exp, (n1, chunks, k))
            kept = top2[TOP2[0]]
            first = got[1][0][kept["index_0"].astype(np.int64), 0]  # k = 1: the row the top-2 list names, wherever it keeps the query
            assert np.array_equal(first["index_1"], kept["index_1"]) and np.array_equal(first["distance"], kept["distance"]), (n1, chunks)
    finally:
        ctx.set_match_mode(2)
        ctx.debug_set_match_chunks(0, 0)
        ctx.set_knn_chunks(0)
