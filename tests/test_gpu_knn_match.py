"""k-nearest-neighbour matching on the GPU (akz_descriptor_match_knn, akz_descriptor_match_knn_device): whole (records, counts)
buffers against the host statement akz_descriptor_match_knn_host, bit for bit -- at the edges of a wave's 32 queries and a
workgroup's 512, of the matcher's LDS tile (T = akz_debug_match_tile_rows, read from the library), for every k and for train
sets shorter than k; with equal distances in both half-lanes of a column, in several sub-tiles, tiles and chunks; across forced
chunk counts; across thresholds; on device-resident rows; and against the existing matcher, an independent path, through the
derivation of descriptor_match from knn(k = 2) that include/akaze_hip.h states."""
import ctypes as C

import numpy as np
import pytest

from test_cross_match_host import planted_sets
from test_knn_match_host import KS, NO_ROW, same, tie_sets

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


def tile_rows(amd):
    rows = C.c_uint32()
    assert amd.lib().akz_debug_match_tile_rows(C.byref(rows)) == 0 and rows.value >= 8
    return rows.value


def rows64(d, fill=0):
    r = np.full((len(d), 64), fill, np.uint8)
    r[:, :d.shape[1]] = d
    return r


def hold(ctx, amd, a, b, k, thr, what):
    exp = amd.descriptor_match_knn_host(a, b, k, thr)
    same(ctx.descriptor_match_knn(a, b, k, thr), exp, what)
    return exp


def device_form(ctx, amd, a64, b64, k, thr):
    """akz_descriptor_match_knn_device into sentinel-filled outputs -> (records (n0, k), counts (n0,)) on the host"""
    import torch
    da, db = torch.from_numpy(a64).cuda(), torch.from_numpy(b64).cuda()
    n0, n1 = len(a64), len(b64)
    out = torch.full((max(n0 * k, 1) * 24,), SENTINEL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((max(n0, 1) * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert amd.lib().akz_descriptor_match_knn_device(ctx._h, C.c_void_p(da.data_ptr()) if n0 else None, n0,
                                                     C.c_void_p(db.data_ptr()) if n1 else None, n1, k, thr,
                                                     C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr())) == 0
    ctx.synchronize()
    rec = out.cpu().numpy()[:n0 * k * 24].copy().view(amd.MATCH_DTYPE).reshape(n0, k)
    return rec, cnt.cpu().numpy()[:n0 * 4].copy().view(np.uint32)


@pytest.fixture(scope="module")
def pool():
    rng = np.random.default_rng(1801)
    return rng.integers(0, 256, (513, 61), dtype=np.uint8), rng.integers(0, 256, (4000, 61), dtype=np.uint8)


@pytest.mark.parametrize("n0", [1, 31, 32, 33, 513])
def test_edges(ctx, amd, pool, n0):
    T = tile_rows(amd)
    a_all, b_all = pool
    for n1 in (1, 3, 7, T - 1, T, T + 1, 2 * T + 5):
        b = b_all[:n1].copy()
        b[n1 // 2] = a_all[0]                                             # (a distance of 0 among the random ones)
        for k in KS:
            exp = hold(ctx, amd, a_all[:n0], b, k, 10000, (n0, n1, k))
            assert np.all(exp[1] == min(k, n1))


@pytest.mark.parametrize("nb", [1, 20])
def test_short_rows(ctx, amd, nb):
    """rows of 1 and 20 bytes: the columns beyond them are zero on both sides (and at 1 byte nearly every distance is a tie)"""
    T = tile_rows(amd)
    rng = np.random.default_rng(1802 + nb)
    a = rng.integers(0, 256, (33, nb), dtype=np.uint8)
    for n1 in (1, 3, 7, T - 1, T, T + 1, 2 * T + 5):
        b = rng.integers(0, 256, (n1, nb), dtype=np.uint8)
        for k in KS:
            hold(ctx, amd, a, b, k, 10000, (nb, n1, k))
            hold(ctx, amd, a, b, k, 3 * nb, (nb, n1, k, "cut"))


def test_empty_sets(ctx, amd, pool):
    a, b = pool[0][:40], pool[1][:50]
    out, counts = hold(ctx, amd, a, b[:0], 3, 10000, "n1 == 0")
    assert np.all(counts == 0) and np.all(out["index_1"] == NO_ROW) and np.all(np.isposinf(out["distance"]))
    rec, cnt = device_form(ctx, amd, rows64(a), rows64(b[:0]), 3, 10000)
    same((rec, cnt), (out, counts), "n1 == 0, device rows")
    assert ctx.descriptor_match_knn(a[:0], b, 3)[0].shape == (0, 3)
    hold(ctx, amd, a, b, 8, 10000, "the call after the empty ones")


def test_ties_across_every_boundary(ctx, amd):
    """3T + 9 train rows from 5 distinct descriptors (row j is descriptor j % 5): a query's equal distances sit in both half-lanes
    of its column, in every sub-tile, tile and chunk -- the kept ones are the lowest rows, whatever the chunking"""
    T = tile_rows(amd)
    a5, b = tie_sets(repeats=(3 * T + 9 + 4) // 5)
    b = b[:3 * T + 9]
    rng = np.random.default_rng(1803)
    a = np.concatenate([a5, rng.integers(0, 256, (40, 61), dtype=np.uint8)])       # (strangers: all their distances near 244)
    exp = amd.descriptor_match_knn_host(a, b, 8)
    for i in range(5):
        assert exp[0]["index_1"][i].tolist() == [i + 5 * r for r in range(8)] and np.all(exp[0]["distance"][i] == 2 * i)
    try:
        for chunks in (1, 2, 3):
            ctx.set_knn_chunks(chunks)
            same(ctx.descriptor_match_knn(a, b, 8), exp, ("chunks", chunks))
            same(ctx.descriptor_match_knn(a, b, 8, 9), amd.descriptor_match_knn_host(a, b, 8, 9), ("chunks", chunks, "threshold 9"))
    finally:
        ctx.set_knn_chunks(0)


def test_chunk_merge(ctx, amd, pool):
    T = tile_rows(amd)
    a, b = pool[0][:70], pool[1][:5 * T + 1]
    try:
        for k in (8, 3):
            exp = amd.descriptor_match_knn_host(a, b, k)
            for chunks in (1, 2, 3, 5, 0):
                ctx.set_knn_chunks(chunks)
                same(ctx.descriptor_match_knn(a, b, k), exp, (k, "chunks", chunks))
    finally:
        ctx.set_knn_chunks(0)


def test_thresholds(ctx, amd):
    """queries and train rows around one centre with flips in disjoint halves of the row: d(i, j) = i + 10 j exactly, so at the
    median threshold the queries keep 0, 1, 2, ... train rows -- every count from 0 to k occurs"""
    rng = np.random.default_rng(1804)
    centre = rng.integers(0, 256, 61, dtype=np.uint8)

    def flipped(first, n):
        row = centre.copy()
        for bit in range(first, first + n):
            row[bit >> 3] ^= np.uint8(1 << (bit & 7))
        return row

    a = np.array([flipped(0, i) for i in range(121)], np.uint8)
    b = np.array([flipped(240, 10 * j) for j in range(12)], np.uint8)
    dist = np.arange(121)[:, None] + 10 * np.arange(12)[None, :]
    median = int(np.median(dist))
    for k in (8, 2):
        for thr in (0, 1, median, 489, 10000):
            out, counts = hold(ctx, amd, a, b, k, thr, (k, thr))
            want = np.minimum(k, (dist < thr).sum(axis=1))
            assert np.array_equal(counts, want), (k, thr)
            for i in (0, 60, 120):
                assert out["distance"][i, :counts[i]].tolist() == [i + 10 * j for j in range(counts[i])]
                assert np.all(out["index_1"][i, counts[i]:] == NO_ROW) and np.all(np.isposinf(out["distance"][i, counts[i]:]))
        if k == 8:
            assert set(np.minimum(8, (dist < median).sum(axis=1)).tolist()) == set(range(9))


def test_device_form(ctx, amd, pool):
    T = tile_rows(amd)
    a, b = pool[0][:300], pool[1][:T + 37]
    for k in (1, 5, 8):
        for thr in (10000, 240):
            exp = hold(ctx, amd, a, b, k, thr, (k, thr))
            same(device_form(ctx, amd, rows64(a), rows64(b), k, thr), exp, (k, thr, "device rows"))       # every slot overwritten
            same(device_form(ctx, amd, rows64(a, 0xFF), rows64(b, 0x3C), k, thr), exp, (k, thr, "garbage in bytes 61..63"))
    import torch
    rec, cnt = ctx.descriptor_match_knn_device(torch.from_numpy(rows64(a)).cuda(), torch.from_numpy(rows64(b)).cuda(), 4)
    ctx.synchronize()
    exp = amd.descriptor_match_knn_host(a, b, 4)
    assert rec.shape == (300, 4, 24) and cnt.shape == (300,)
    same((rec.cpu().numpy().view(amd.MATCH_DTYPE).reshape(300, 4), cnt.cpu().numpy().view(np.uint32)), exp, "the binding")


def derived_match(amd, out, counts, thr, ratio):
    """descriptor_match from knn(k = 2, thr), as include/akaze_hip.h derives it"""
    keep = []
    for i in range(len(out)):
        mn = out["distance"][i, 0] if counts[i] >= 1 else float(thr)
        second = out["distance"][i, 1] if counts[i] == 2 else float(thr)
        if float(mn) < float(second) * (ratio * ratio) and mn < thr:
            keep.append(i)
    res = np.zeros(len(keep), amd.MATCH_DTYPE)
    keep = np.array(keep, np.int64)
    res["index_0"], res["index_1"], res["distance"] = keep, out["index_1"][keep, 0], out["distance"][keep, 0]
    return res


def test_agrees_with_descriptor_match(ctx, amd):
    a, b = planted_sets(1805, 61, mutual=1200, rival=50, reverse_ratio=50, tie=50, orphan=50, stranger=100)[:2]
    assert 1500 <= len(a) <= 1700
    full = None
    for thr in (10000, 8):
        out, counts = ctx.descriptor_match_knn(a, b, 2, thr)
        for ratio in (0.86, 1.0):
            exp = ctx.descriptor_match(a, b, thr, ratio)
            got = derived_match(amd, out, counts, thr, ratio)
            assert got.dtype == exp.dtype and np.array_equal(got, exp), (thr, ratio, len(got), len(exp))
            assert len(exp) > 0
            if thr == 10000 and ratio == 0.86:
                full = len(exp)
        if thr == 8:
            assert len(ctx.descriptor_match(a, b, thr, 0.86)) < full                 # the threshold cuts the list


def test_one_larger_shape(ctx, amd, pool):
    rng = np.random.default_rng(1806)
    a = rng.integers(0, 256, (3000, 61), dtype=np.uint8)
    hold(ctx, amd, a, pool[1], 8, 10000, "3000 x 4000")


def test_refusals(ctx, amd, pool):
    a, b = pool[0][:50], pool[1][:60]
    L = amd.lib()
    out = np.zeros((50, 8), amd.MATCH_DTYPE)
    out["index_0"] = 77
    counts = np.full(50, 4242, np.uint32)
    wide = np.zeros((60, 62), np.uint8)
    for what, rows_a, rows_b, nb, k, status in (("62 bytes", wide[:50], wide, 62, 2, -6), ("k = 0", a, b, 61, 0, -1), ("k = 9", a, b, 61, 9, -1)):
        got = L.akz_descriptor_match_knn(ctx._h, rows_a.ctypes.data, 50, rows_b.ctypes.data, 60, nb, k, 10000, out.ctypes.data, counts.ctypes.data)
        assert got == status, (what, got)
        assert np.all(out["index_0"] == 77) and np.all(counts == 4242), what
        hold(ctx, amd, a, b, 2, 10000, ("the call after", what))
    import torch
    da, db = torch.from_numpy(rows64(a)).cuda(), torch.from_numpy(rows64(b)).cuda()
    d_out = torch.full((50 * 8 * 24,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((50 * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    for k in (0, 9):
        assert L.akz_descriptor_match_knn_device(ctx._h, C.c_void_p(da.data_ptr()), 50, C.c_void_p(db.data_ptr()), 60, k, 10000,
                                                 C.c_void_p(d_out.data_ptr()), C.c_void_p(d_cnt.data_ptr())) == -1
    ctx.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_cnt == SENTINEL).all())
