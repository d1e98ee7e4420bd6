"""Every descriptor-matching entry point on the GPU against the numpy statement of tests/match_numpy.py -- not the oracle --, whole
lists as arrays, on the cases of tests/match_cases.py (planted top-2 at every partition edge, one row below the threshold, far
sets, tail bits and padding bytes, the seed boundary of the both-direction form):

  descriptor_match                      every matcher mode (0 popcount, 1 int8 matrix, 2 and 3 FP4), 1, 2, 3 and 5 forced pair chunks
  descriptor_match_device               64-byte rows whose bytes 61 .. 63 hold random data (not compared)
  descriptor_match on 64-byte rows      the host entry point: every byte counts
  descriptor_match_sets_device          all train sets of a case in one launch, an empty and a one-row set among them, 1, 2 and 3
                                        forced set chunks
  descriptor_match_sets_mutual_device   both directions, on the seed-boundary cases and on the planted and far ones
  descriptor_match_cross, descriptor_match_knn (k = 1, 2, 8; 1, 2, 3, 5 chunks), descriptor_match_guided with a gate that admits
  every row (identity homography, all keypoints at one point, radius 1)

Nothing here takes a tolerance: indices, counts and f64 distances that are integers, compared as arrays.  What each case can
see -- the switches and simulated kernel faults it catches -- is shown without a GPU in tests/test_match_statement_host.py."""
import numpy as np
import pytest

import match_cases as MC
import match_numpy as M

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3)
PAIR_CASES = ("planted33", "planted513", "lone33", "far33", "far513", "tail33", "seed0", "seed1", "seed2")
FAMILIES = ("planted33", "planted513", "far33", "far513", "lone33", "tail33")


@pytest.fixture(scope="module")
def world(amd):
    """the cases and, computed once and left unchanged, what the statement says about them"""
    g = MC.geometry(amd)
    cases, _ = MC.all_cases(g)
    fwd, rev = {}, {}
    for case in cases.values():
        d0 = case.d0[:, :61] if case.name.startswith("padded64") else case.d0
        for k, d1 in enumerate(case.sets):
            fwd[(case.name, k)] = M.match_settings(M.distances(d0, d1[:, :d0.shape[1]]), case.settings)
            assert any(0 < len(m) < len(d0) for m in fwd[(case.name, k)].values()) or len(d1) <= 3, (case.name, k)   # never only empty or full lists
            if case.name.startswith("seed") or k < 3 or len(d1) < 4:
                rev[(case.name, k)] = M.match_settings(M.distances(d1[:, :d0.shape[1]], d0), case.settings)
    return g, cases, fwd, rev


def same(got, exp, what):
    assert got.dtype == exp.dtype and np.array_equal(got, exp), (what, len(got), len(exp))


def rows64(d, rng):
    """64-byte rows: the descriptor bytes, then RANDOM bytes where the device forms compare nothing"""
    r = rng.integers(0, 256, (len(d), 64), dtype=np.uint8)
    r[:, :min(d.shape[1], 61)] = d[:, :61]
    return r


def device_list(amd, out, cnt, cap):
    n = int(cnt)
    assert 0 <= n <= cap
    return out[:n].copy().view(amd.MATCH_DTYPE).reshape(-1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", PAIR_CASES)
def test_descriptor_match(ctx, amd, world, name, mode):
    _, cases, fwd, _ = world
    case = cases[name]
    try:
        ctx.set_match_mode(mode)
        for chunks in MC.CHUNKS if mode else (1,):                       # (the popcount kernel cuts its chunks itself)
            ctx.debug_set_match_chunks(chunks, 0)
            for k, d1 in enumerate(case.sets):
                for (thr, ratio), exp in fwd[(name, k)].items():
                    same(ctx.descriptor_match(case.d0, d1, thr, ratio), exp, (name, mode, chunks, len(d1), thr, ratio))
    finally:
        ctx.set_match_mode(2)
        ctx.debug_set_match_chunks(0, 0)


@pytest.mark.parametrize("mode", MODES)
def test_host_entry_point_compares_every_byte(ctx, amd, world, mode):
    """64-byte rows through akz_descriptor_match: bytes 61 .. 63 count (the statement on all 64 bytes)"""
    _, cases, _, _ = world
    case = cases["padded64_33"]
    d1 = case.sets[0]
    exp = M.match_settings(M.distances(case.d0, d1), case.settings)
    moved = 0
    try:
        ctx.set_match_mode(mode)
        for (thr, ratio), e in exp.items():
            same(ctx.descriptor_match(case.d0, d1, thr, ratio), e, (mode, thr, ratio))
            moved += not np.array_equal(e, M.descriptor_match(case.d0[:, :61], d1[:, :61], thr, ratio))
    finally:
        ctx.set_match_mode(2)
    assert moved >= 2                                                    # the padding bytes do change these lists


@pytest.mark.parametrize("mode", MODES)
def test_descriptor_match_device(ctx, amd, world, mode):
    import torch
    _, cases, fwd, _ = world
    rng = np.random.default_rng(61)
    try:
        ctx.set_match_mode(mode)
        for name in ("planted33", "lone33", "far33", "tail33", "padded64_33", "seed0"):
            case = cases[name]
            dq = torch.from_numpy(rows64(case.d0, rng) if case.d0.shape[1] == 61 else case.d0).cuda()
            for k, d1 in enumerate(case.sets[:5]):
                dt = torch.from_numpy(rows64(d1, rng) if d1.shape[1] == 61 else d1).cuda()
                for (thr, ratio), exp in fwd[(name, k)].items():
                    out, cnt = ctx.descriptor_match_device(dq, dt, thr, ratio)
                    ctx.synchronize()
                    same(device_list(amd, out.cpu().numpy(), cnt.item(), len(case.d0)), exp, (name, mode, len(d1), thr, ratio))
    finally:
        ctx.set_match_mode(2)


def family(case, rng):
    """the train sets of a case for one launch, an EMPTY set and a ONE-ROW set (the first row of the first set) among them ->
    (rows per set, all rows, index into case.sets or "one" / "empty" per launched set)"""
    which = list(range(len(case.sets)))
    which.insert(1, "empty")
    which.insert(min(3, len(which)), "one")
    sets = [case.sets[w] if isinstance(w, int) else case.sets[0][:1 if w == "one" else 0] for w in which]
    return [len(s) for s in sets], np.concatenate([rows64(s, rng) for s in sets]), which, sets


@pytest.mark.parametrize("mode", (1, 2, 3))
@pytest.mark.parametrize("name", FAMILIES)
def test_descriptor_match_sets_device(ctx, amd, world, name, mode):
    import torch
    _, cases, fwd, _ = world
    case = cases[name]
    rng = np.random.default_rng(62)
    rows, cat, which, sets = family(case, rng)
    dq, dcat = torch.from_numpy(rows64(case.d0, rng)).cuda(), torch.from_numpy(cat).cuda()
    one = M.match_settings(M.distances(case.d0, case.sets[0][:1]), case.settings)
    try:
        ctx.set_match_mode(mode)
        for chunks in (1, 2, 3):
            ctx.debug_set_match_chunks(0, chunks)
            for thr, ratio in case.settings[:8]:
                out, cnt = ctx.descriptor_match_sets_device(dq, dcat, rows, thr, ratio)
                ctx.synchronize()
                out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
                for s, w in enumerate(which):
                    exp = fwd[(name, w)][(thr, ratio)] if isinstance(w, int) else (one[(thr, ratio)] if w == "one" else np.zeros(0, M.MATCH_DTYPE))
                    same(device_list(amd, out[s], cnt[s], len(case.d0)), exp, (name, mode, chunks, s, w, thr, ratio))
    finally:
        ctx.set_match_mode(2)
        ctx.debug_set_match_chunks(0, 0)


@pytest.mark.parametrize("mode", (2, 1))
@pytest.mark.parametrize("name", ("seed0", "seed1", "seed2", "planted33", "planted513", "far33"))
def test_descriptor_match_sets_mutual_device(ctx, amd, world, name, mode):
    """both directions from one launch; mode 1 takes the opposite direction pair by pair (the other kernels have no such form)"""
    import torch
    _, cases, fwd, rev = world
    case = cases[name]
    rng = np.random.default_rng(63)
    keep = [k for k in range(len(case.sets)) if (name, k) in rev]
    sets = [case.sets[k] for k in keep] + [case.sets[0][:0]]
    rows = [len(s) for s in sets]
    dq = torch.from_numpy(rows64(case.d0, rng)).cuda()
    dcat = torch.from_numpy(np.concatenate([rows64(s, rng) for s in sets])).cuda()
    offs = np.concatenate([[0], np.cumsum(rows)])
    try:
        ctx.set_match_mode(mode)
        for chunks in (1, 3) if mode == 2 else (1,):
            ctx.debug_set_match_chunks(0, chunks)
            for thr, ratio in case.settings:
                out, cnt, cout, ccnt = ctx.descriptor_match_sets_mutual_device(dq, dcat, rows, thr, ratio)
                ctx.synchronize()
                out, cnt, cout, ccnt = out.cpu().numpy(), cnt.cpu().numpy(), cout.cpu().numpy(), ccnt.cpu().numpy()
                for s, k in enumerate(keep):
                    what = (name, mode, chunks, len(sets[s]), thr, ratio)
                    same(device_list(amd, out[s], cnt[s], len(case.d0)), fwd[(name, k)][(thr, ratio)], what + ("query direction",))
                    same(device_list(amd, cout[offs[s]:offs[s + 1]], ccnt[s], rows[s]), rev[(name, k)][(thr, ratio)], what + ("opposite direction",))
                assert cnt[len(keep)] == 0 and ccnt[len(keep)] == 0       # the empty set
    finally:
        ctx.set_match_mode(2)
        ctx.debug_set_match_chunks(0, 0)


@pytest.mark.parametrize("mode", (2, 1, 0))
def test_descriptor_match_cross(ctx, amd, world, mode):
    _, cases, fwd, rev = world
    try:
        ctx.set_match_mode(mode)
        for name in ("planted33", "lone33", "far33", "tail33", "seed0", "seed1"):
            case = cases[name]
            for k, d1 in enumerate(case.sets[:3]):
                for (thr, ratio), f in fwd[(name, k)].items():
                    exp = M.cross_filter(f, rev[(name, k)][(thr, ratio)])
                    same(ctx.descriptor_match_cross(case.d0, d1, thr, ratio), exp, (name, mode, len(d1), thr, ratio))
    finally:
        ctx.set_match_mode(2)


@pytest.mark.parametrize("name", ("planted33", "planted513", "lone33", "far33", "tail33"))
def test_descriptor_match_knn(ctx, amd, world, name):
    _, cases, _, _ = world
    case = cases[name]
    try:
        for d1 in case.sets[:3] + case.sets[-1:]:
            dist = M.distances(case.d0, d1)
            thrs = sorted({t for t, _ in case.settings})
            exp = {(k, thr): M.knn(case.d0, d1, k, thr, dist) for k in (1, 2, 8) for thr in (thrs[2:5] if len(thrs) > 3 else thrs)}
            for chunks in MC.CHUNKS:
                ctx.set_knn_chunks(chunks)
                for (k, thr), (e_out, e_cnt) in exp.items():
                    out, cnt = ctx.descriptor_match_knn(case.d0, d1, k, thr)
                    assert cnt.dtype == np.uint32 and np.array_equal(cnt, e_cnt), (name, len(d1), chunks, k, thr, "counts")
                    assert out.dtype == e_out.dtype and out.tobytes() == e_out.tobytes(), (name, len(d1), chunks, k, thr, "records")
    finally:
        ctx.set_knn_chunks(0)
    if name == "far33":                                                  # k = 8 against three rows: three entries, five empty slots
        out, cnt = ctx.descriptor_match_knn(case.d0, case.sets[1], 8, MC.BIG)
        assert len(case.sets[1]) == 3 and np.all(cnt == 3) and np.all(out["index_1"][:, 3:] == M.NO_ROW)


@pytest.mark.parametrize("name", ("planted33", "lone33", "far33", "tail33", "seed1"))
def test_descriptor_match_guided_with_every_row_admitted(ctx, amd, world, name):
    """identity homography, every keypoint at one point, radius 1: w = 1, du = dv = 0 < 1 -- the gate admits every row, and the
    guided scan is the blind one"""
    _, cases, fwd, _ = world
    case = cases[name]

    def at_one_point(n):
        k = np.zeros(n, amd.KEYPOINT_DTYPE)
        k["x"], k["y"] = 10.0, 20.0
        return k

    for k, d1 in enumerate(case.sets[:4]):
        for (thr, ratio), exp in fwd[(name, k)].items():
            got = amd.descriptor_match_guided(at_one_point(len(case.d0)), case.d0, at_one_point(len(d1)), d1, np.eye(3), amd.GUIDED_HOMOGRAPHY, 1.0,
                                              thr, ratio, ctx=ctx)
            same(got, exp, (name, len(d1), thr, ratio))
