"""Descriptor sets placed at the edges of the matching kernels, for tests/test_match_statement_host.py (no GPU) and
tests/test_gpu_match_statement.py.  Every builder checks its own premise with the numpy statement (tests/match_numpy.py) before
it returns: the planted rows ARE the minimum and the second, and every unplanted row is farther away than the largest planted
second.

What the kernels partition a train set by (geometry(): read from the library and the source, so a retuned kernel moves the cases):
  T     rows per LDS tile of the matrix-core matchers (akz_debug_match_tile_rows); k_match_fp4 walks two tiles per step, and a
        lane holds rows (i & 3) + 8 (i >> 2) + 4 h of every 32-row sub-tile (fp4::lane_row; h: the half-lane);
  MT    rows per LDS tile of the popcount kernel k_match, which feeds four rows per iteration and the remainder one by one;
  seed  the query rows that seed the opposite direction of the both-direction form (akz_debug_match_seed_rows); the rows from
        there on enter through atomicMin on cbest / csecond;
  the chunk cut of launch::match_mfma and match_sets_impl: ceil(tiles / chunks) tiles per chunk.

A Case is (name, d0, sets, settings): one query set, a family of train sets (matched one by one by the pair calls and all at once
by the multi-set launch) and the (threshold, ratio) settings it is run at."""
import ctypes as C
import math
import os
import re
from collections import namedtuple

import numpy as np

import match_numpy as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Case = namedtuple("Case", "name d0 sets settings")
Geometry = namedtuple("Geometry", "T MT unroll seed_tiles")

RATIO_HALF = 0.5                      # 0.25 exactly: m < 4 m * 0.25 is an equality
RATIO_SQRT_HALF = math.sqrt(0.5)      # ratio * ratio = 0.5000000000000001 in f64, 0.49999997 in f32
BIG = 10000
THRESHOLDS = (0, 1, 489, BIG, 2 ** 31 - 1, 2 ** 31, 2 ** 63 - 1)
CHUNKS = (1, 2, 3, 5)
MAX_M = 24                            # planted minima are 1 .. MAX_M bits, planted seconds at most 4 MAX_M + 1 = 97
FAR_FROM = 4 * MAX_M + 1
KINDS = ("4m", "4m+1", "tie", "2m", "4m", "4m+1", "tie")


def geometry(amd):
    rows = C.c_uint32()
    assert amd.lib().akz_debug_match_tile_rows(C.byref(rows)) == 0 and rows.value >= 32 and rows.value % 32 == 0
    T = rows.value
    seed = C.c_uint32()
    assert amd.lib().akz_debug_match_seed_rows(1 << 30, C.byref(seed)) == 0 and seed.value % T == 0 and seed.value >= T
    assert amd.lib().akz_debug_match_seed_rows(5, C.byref(rows)) == 0 and rows.value == 5       # a short query set seeds whole
    src = open(os.path.join(ROOT, "akaze-rust_amd", "csrc", "akz_kernels.hip")).read()
    body = src[src.index("Brute-force Hamming 1-NN / 2-NN"):src.index("k_match_merge(")]
    mt = int(re.search(r"constexpr int MT = (\d+);", body).group(1))
    unroll = int(re.search(r"for \(; r \+ (\d+) <= rows; r \+= \1\)", body).group(1))
    return Geometry(T, mt, unroll, seed.value // T)


def lane_half(row):
    """the half-lane h of a train row (rows (i & 3) + 8 (i >> 2) + 4 h of a 32-row sub-tile)"""
    return (row >> 2) & 1


def chunk_of(row, n1, chunks, T):
    """the chunk of a train row under launch::match_mfma / match_sets_impl"""
    tiles = max(1, -(-n1 // T))
    chunks = max(1, min(chunks, tiles))
    return (row // T) // (-(-tiles // chunks))


def flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def second_bits(kind, m):
    return {"4m": 4 * m, "4m+1": 4 * m + 1, "tie": m, "2m": 2 * m}[kind]


def probe_rows(rng, q, kind, m, bits=480):
    """(row at m bits from q, row at the kind's second distance from q, on other bits)"""
    order = rng.permutation(bits)
    s = second_bits(kind, m)
    return flip(q, order[:m]), flip(q, order[m:m + s])


def edge_rows(g, n1):
    T, e = g.T, set()
    e.update((0, 1, 3, 4, 5, 7, 8, 12, 15, 16, 28, 31, 32, 35, 36, 63, 64, 95, 96))
    e.update((T - 5, T - 4, T - 1, T, T + 1, T + 4, 2 * T - 1, 2 * T, 2 * T + 3, 2 * T + 4))
    tiles = -(-n1 // T)
    for chunks in CHUNKS + (2,):                                     # (2: the step of two tiles cuts where two chunks do not)
        per = -(-tiles // min(chunks, tiles))
        for c in range(1, tiles):
            if c % per == 0 or c % 2 == 0:
                e.update((c * T - 1, c * T, c * T + 4))
    for k in range(1, n1 // g.MT + 1):                                # the popcount kernel's tiles
        e.update((k * g.MT - 1, k * g.MT))
    e.update((n1 - 1, n1 - 2, n1 - g.unroll, n1 - g.unroll - 1))
    return sorted(r for r in e if 0 <= r < n1)


# ---- planted top-2 -----------------------------------------------------------------------------------------------------------
def planted_pairs(g, n1):
    """(p, s, kind): the minimum's row, the second's row, the second's distance -- neighbours in the list of edges (the two
    sides of every boundary), then rows 5 and 13 edges apart (other sub-tiles, tiles, steps and chunks), every tie in both
    orders, and the pairs that tell the two half-lanes of a column apart"""
    E = edge_rows(g, n1)[:-1]                                            # (the last row has a probe of its own in every set)
    out, k = [], 0
    for off in (1, 5, 13):
        for a in range(len(E)):
            p, s = E[a], E[(a + off) % len(E)]
            kind = KINDS[k % len(KINDS)]
            k += 1
            out.append((p, s, kind))
            if kind == "tie" or off == 1:
                out.append((s, p, kind))
    T = g.T
    for lo, hi in ((4, 8), (5, 16), (7, 32), (12, T), (15, 2 * T), (T + 4, T + 8), (T - 4, T), (28, 32)):
        out += [(lo, hi, "tie"), (hi, lo, "tie"), (lo, hi, "4m"), (hi, lo, "4m+1")]
    return out


def planted(g, n0, seed=1):
    """The planted top-2 family: query i of a train set carries one (p, s); the train sets (of 5 T + 1, 5 T, 5 T - 1 and 5 T - 2
    rows: n1 = 1, 0, 3, 2 mod 4) carry the pairs between them, and each has a probe on its last row."""
    rng = np.random.default_rng(seed * 1000 + n0)
    T = g.T
    d0 = rng.integers(0, 256, (n0, 61), dtype=np.uint8)
    sizes = (5 * T + 1, 5 * T, 5 * T + 1, 5 * T - 1, 5 * T + 1, 5 * T - 2)
    todo = planted_pairs(g, 5 * T + 1)
    sets, plans = [], []
    while todo and len(sets) < 20:
        n1 = sizes[len(sets) % len(sizes)]
        d1 = rng.integers(0, 256, (n1, 61), dtype=np.uint8)
        used, plan, rest = set(), [], []
        first = (n1 - 1, (7 * len(sets)) % 97, "4m") if len(sets) % 2 == 0 else ((11 * len(sets)) % 97, n1 - 1, "4m+1")
        for p, s, kind in [first] + todo:
            if len(plan) < n0 and p < n1 and s < n1 and p != s and p not in used and s not in used:
                used.update((p, s))
                plan.append((p, s, kind))
            elif (p, s, kind) != first:
                rest.append((p, s, kind))
        for i, (p, s, kind) in enumerate(plan):
            m = 1 + (i + 5 * len(sets)) % MAX_M
            d1[p], d1[s] = probe_rows(rng, d0[i], kind, m)
        todo = rest
        sets.append(d1)
        plans.append(plan)
    assert not todo, len(todo)
    settings = ((BIG, RATIO_HALF), (BIG, 1.5), (BIG, RATIO_SQRT_HALF), (489, 1.0))
    case = Case(f"planted{n0}", d0, sets, settings)
    _check_planted(g, case, plans)
    return case, plans


def _check_planted(g, case, plans):
    seen = set()
    for d1, plan in zip(case.sets, plans):
        dist = M.distances(case.d0, d1)
        for i, (p, s, kind) in enumerate(plan):
            m = int(dist[i, p])
            assert 1 <= m <= MAX_M and dist[i, s] == second_bits(kind, m), (case.name, i, p, s, kind)
            others = np.delete(dist[i], [p, s])
            assert others.min() > FAR_FROM, (case.name, i, int(others.min()))
        if len(plan) < len(case.d0):
            assert dist[len(plan):].min() > FAR_FROM
        # what the settings must say about the probes (the statement's own lists are compared with these)
        lists = M.match_settings(dist, ((BIG, RATIO_HALF), (BIG, 1.5), (BIG, RATIO_SQRT_HALF)))
        half, wide, root = lists[(BIG, RATIO_HALF)], lists[(BIG, 1.5)], lists[(BIG, RATIO_SQRT_HALF)]
        kept_half, kept_root = set(half["index_0"].tolist()), set(root["index_0"].tolist())
        name = dict(zip(wide["index_0"].tolist(), wide["index_1"].tolist()))
        for i, (p, s, kind) in enumerate(plan):
            assert (i in kept_half) == (kind == "4m+1"), (case.name, i, kind)          # 4m: an equality, rejected
            assert (i in kept_root) == (kind != "tie"), (case.name, i, kind)           # 2m: kept by 0.5000000000000001 alone
            assert name[i] == (min(p, s) if kind == "tie" else p), (case.name, i, kind)
            seen.add((lane_half(p) == lane_half(s), p // 32 == s // 32, p // g.T == s // g.T, p // (2 * g.T) == s // (2 * g.T), kind))
    # minimum and second in the same half-lane, in the two half-lanes of one column, in different sub-tiles, tiles and steps
    for kind in ("4m", "4m+1", "tie"):
        for where in ((True, True, True, True), (False, True, True, True), (True, False, True, True), (True, False, False, True),
                      (True, False, False, False), (False, False, False, False)):
            assert where + (kind,) in seen, (case.name, where, kind)
    for d1, plan in zip(case.sets, plans):                              # and in different chunks under every forced count
        for chunks in CHUNKS[1:]:
            assert any(chunk_of(p, len(d1), chunks, g.T) != chunk_of(s, len(d1), chunks, g.T) for p, s, _ in plan)
    assert {len(d1) % 4 for d1 in case.sets} == {0, 1, 2, 3}
    assert all(any(len(d1) - 1 in (p, s) for p, s, _ in plan) for d1, plan in zip(case.sets, plans))


# ---- one row below the threshold ----------------------------------------------------------------------------------------------
LONE_M0 = 12
LONE_MS = (0, LONE_M0 - 1, LONE_M0, LONE_M0 + 1, 4 * LONE_M0 - 1, 4 * LONE_M0, 4 * LONE_M0 + 1)


def lone(g, n0=33, seed=2):
    """Every query has ONE train row within 4 M0 + 1 bits (at m = 0, M0 - 1, M0, M0 + 1, 4 M0 - 1, 4 M0, 4 M0 + 1 bits, on the
    edge rows), every other row is a random one: at thresholds 4 M0 and 4 M0 + 1 the second stays AT the threshold, and the
    ratio test runs against it -- at ratio 0.5, m = M0 is rejected by thr = 4 M0 (an equality) and kept by 4 M0 + 1; m == thr
    is never a match, m == thr - 1 is one from ratio 1 on."""
    rng = np.random.default_rng(seed * 1000 + n0)
    T = g.T
    n1 = 2 * T + 1
    d0 = rng.integers(0, 256, (n0, 61), dtype=np.uint8)
    d1 = rng.integers(0, 256, (n1, 61), dtype=np.uint8)
    rows = edge_rows(g, n1)[::-1]                                        # the last row first; then rows anywhere
    rows += [int(r) for r in rng.permutation(n1) if r not in rows]
    ms = [LONE_MS[i % len(LONE_MS)] for i in range(n0)]
    for i in range(n0):
        d1[rows[i]] = flip(d0[i], rng.permutation(480)[:ms[i]])
    thr_lo, thr_hi = 4 * LONE_M0, 4 * LONE_M0 + 1
    settings = tuple((thr, r) for thr in (thr_lo, thr_hi) for r in (RATIO_HALF, 1.0, 1.5)) + tuple((thr, r) for thr in THRESHOLDS for r in (RATIO_HALF, 1.5))
    case = Case(f"lone{n0}", d0, [d1], settings)
    dist = M.distances(d0, d1)
    for i in range(n0):
        assert dist[i, rows[i]] == ms[i] and np.delete(dist[i], rows[i]).min() > FAR_FROM
    for thr in (thr_lo, thr_hi):
        mn, second, _ = M.top2(dist, thr)
        assert np.all(second == thr)                                    # the second stays at the threshold for every query
        for ratio in (RATIO_HALF, 1.0, 1.5):
            kept = set(M.descriptor_match(d0, d1, thr, ratio)["index_0"].tolist())
            for i, m in enumerate(ms):
                assert (i in kept) == (m < thr and m < thr * ratio * ratio), (thr, ratio, i, m)
    kept = {thr: {ms[i] for i in M.descriptor_match(d0, d1, thr, RATIO_HALF)["index_0"].tolist()} for thr in (thr_lo, thr_hi)}
    assert LONE_M0 not in kept[thr_lo] and LONE_M0 in kept[thr_hi]
    return case


# ---- far sets ------------------------------------------------------------------------------------------------------------------
def far(g, n0=33, seed=3):
    """Queries within 40 bits of a pattern c, train rows within 40 bits of ~c (query 0 is c, train rows 0 and 1 are ~c: distance
    488, the accumulators' extreme, tied): every distance is at least 408, so a padding row of a partial tile that takes part --
    at 244, an all-zero FP4 row, or at |query|, an all-zero int8 row -- wins."""
    rng = np.random.default_rng(seed * 1000 + n0)
    T = g.T
    c = rng.integers(0, 256, 61, dtype=np.uint8)
    d0 = np.array([flip(c, rng.permutation(488)[:rng.integers(0, 41) if i else 0]) for i in range(n0)], np.uint8)
    sets = []
    for n1 in (1, 3, T - 1, T + 1, 2 * T + 1):
        sets.append(np.array([flip(~c, rng.permutation(488)[:rng.integers(0, 41) if j > 1 else 0]) for j in range(n1)], np.uint8))
    case = Case(f"far{n0}", d0, sets, ((489, 1.0), (489, 1.5), (BIG, 1.0), (BIG, 1.5)))
    for d1 in sets:
        dist = M.distances(d0, d1)
        assert dist.min() >= 408 and dist[0, 0] == 488 and (len(d1) < 2 or dist[0, 1] == 488)
        assert np.all(np.unpackbits(d0, axis=1).sum(1) < 408)           # |q| < every distance: an all-zero row would win
    return case


# ---- tail bits and padding bytes -----------------------------------------------------------------------------------------------
def tail_bits(g, n0=33, seed=4):
    """Rows that differ from their query only in bits 486 and 487 (the last two of the 488 the matrix forms carry; M-LDB fills
    486): query i has row a at one LOW bit and row b at bits 486 + 487 (2 bits) -- a matcher that drops the two bits sees b at
    distance 0 and names it; every third query has its tie between bit 486 and bit 487 alone."""
    rng = np.random.default_rng(seed * 1000 + n0)
    n1 = g.T + 1
    d0 = rng.integers(0, 256, (n0, 61), dtype=np.uint8)
    d1 = rng.integers(0, 256, (n1, 61), dtype=np.uint8)
    rows = rng.permutation(n1)[:2 * n0].reshape(n0, 2)
    for i, (a, b) in enumerate(rows):
        if i % 3 == 2:
            d1[a], d1[b] = flip(d0[i], [486]), flip(d0[i], [487])
        else:
            d1[a], d1[b] = flip(d0[i], [int(rng.integers(0, 480))]), flip(d0[i], [486, 487])
    case = Case(f"tail{n0}", d0, [d1], ((BIG, RATIO_HALF), (BIG, 1.5), (BIG, 1.0), (2, 1.5)))
    dist = M.distances(d0, d1)
    for i, (a, b) in enumerate(rows):
        assert (dist[i, a], dist[i, b]) == ((1, 1) if i % 3 == 2 else (1, 2)) and np.delete(dist[i], [a, b]).min() > FAR_FROM
    return case


def padded64(g, n0=33, seed=5):
    """64-byte rows whose bytes 61 .. 63 hold random data: the host entry points compare every byte, the device entry points
    take them as M-LDB rows and do not compare bytes 61 .. 63 (include/akaze_hip.h).  Query i has row a at m bits and row b at
    m + 2 bits of the first 61 bytes; the 24 random padding bits (about 12 +- 2.4 differ) reorder them for the host forms.
    -> (case, rows): the case holds the 64-byte rows; the statement of a device call is the statement on rows[:, :61]."""
    rng = np.random.default_rng(seed * 1000 + n0)
    n1 = g.T + 1
    d0 = rng.integers(0, 256, (n0, 64), dtype=np.uint8)
    d1 = rng.integers(0, 256, (n1, 64), dtype=np.uint8)
    rows = rng.permutation(n1)[:2 * n0].reshape(n0, 2)
    for i, (a, b) in enumerate(rows):
        m = 1 + i % MAX_M
        order = rng.permutation(480)
        pa, pb = d1[a, 61:].copy(), d1[b, 61:].copy()
        d1[a], d1[b] = flip(d0[i], order[:m]), flip(d0[i], order[m:2 * m + 2])
        d1[a, 61:], d1[b, 61:] = pa, pb
    case = Case(f"padded64_{n0}", d0, [d1], ((BIG, 1.0), (BIG, 1.5), (BIG, 0.9), (40, 1.5)))
    dist61 = M.distances(d0[:, :61], d1[:, :61])
    for i, (a, b) in enumerate(rows):
        m = 1 + i % MAX_M
        assert (dist61[i, a], dist61[i, b]) == (m, m + 2) and np.delete(dist61[i], [a, b]).min() > FAR_FROM
    return case


# ---- the seed boundary of the both-direction form -----------------------------------------------------------------------------
def seed_queries(seed_rows, n0):
    return [q for q in (0, 31, 32, 511, 512, seed_rows - 1, seed_rows, seed_rows + 1, seed_rows + 31, seed_rows + 32, seed_rows + 511,
                        seed_rows + 512, n0 - 1) if 0 <= q < n0]


def seed_plans(seed_rows, n0):
    """One list per case of (qa, qb, qc, kind) per train row: its minimum's and its second's QUERY index (qc: a third row at
    the same distance, or None).  Over the three cases every kind has its two rows on the seed side, beyond the seed, and one on
    either side in both orders; pairs sit in one wave, in neighbouring waves, at the two ends of a 512-query block and across two
    blocks; the triple ties (all in the first case) have their lowest index where a parallel form meets it last."""
    s, last = seed_rows, n0 - 1
    assert sorted({0, 31, 32, 511, 512, s - 1, s, s + 1, s + 31, s + 32, s + 511, s + 512, last}) == sorted(set(seed_queries(s, n0)))
    triples = [(s + 2, s + 40, s + 300, "tie"), (s + 64, s + 200, s + 450, "tie"), (s + 5, s + 508, s + 510, "tie"),
               (s - 2, s + 3, s + 400, "tie"), (510, s + 6, s + 509, "tie"), (s + 65, s + 66, s + 67, "tie")]
    return [triples + [(0, 31, None, "4m"), (s - 1, s, None, "tie"), (s + 1, 32, None, "4m+1"), (s + 31, s + 32, None, "4m"),
                       (s + 511, last, None, "tie"), (511, 512, None, "4m+1")],
            [(s - 1, s, None, "4m"), (last, 0, None, "tie"), (31, 32, None, "tie"), (s + 1, s + 31, None, "4m+1"),
             (s + 32, 511, None, "4m"), (512, s + 511, None, "4m+1")],
            [(s, s - 1, None, "4m+1"), (0, last, None, "2m"), (s + 1, s + 511, None, "tie"), (32, 31, None, "4m"),
             (s + 32, s + 31, None, "tie"), (512, 511, None, "2m")]]


def seed_boundary(g, seed=6):
    """n0 = seed rows + 513 queries against a train set of 5 T + 1 rows (the later cases: 2 T + 1); the probes are planted in the
    QUERY set, for the train rows as queries of the opposite direction: train row t has its minimum at query qa and its second
    at query qb, over the queries on both sides of the seed boundary and of the 512-query blocks.  A query index carries one
    probe, so the plans are spread over three cases (each its own query set).  The last train row of every case has ONE query
    below threshold 150, and that one lies beyond the seed.  -> [(case, plan)], plan = [(t, qa, qb, qc, kind)]"""
    T, seed_rows = g.T, g.seed_tiles * g.T
    n0 = seed_rows + 513
    out = []
    for v, pairs in enumerate(seed_plans(seed_rows, n0)):
        rng = np.random.default_rng(seed * 1000 + v)
        n1 = 5 * T + 1 if v == 0 else 2 * T + 1                          # (one case at the largest size, the others smaller)
        train_rows = [r for r in edge_rows(g, n1) if r != n1 - 1]
        d0 = rng.integers(0, 256, (n0, 61), dtype=np.uint8)
        d1 = rng.integers(0, 256, (n1, 61), dtype=np.uint8)
        lone_q = seed_rows + 100
        used = [q for pr in pairs for q in pr[:3] if q is not None] + [lone_q]
        assert len(used) == len(set(used)) and len(pairs) <= len(train_rows)
        plan = [(train_rows[(5 * k + 3 * v) % len(train_rows)],) + pr for k, pr in enumerate(pairs)]
        assert len({p[0] for p in plan}) == len(plan)
        for k, (t, qa, qb, qc, kind) in enumerate(plan):
            m = 1 + (k + 7 * v) % MAX_M
            d0[qa], d0[qb] = probe_rows(rng, d1[t], kind, m)
            if qc is not None:
                d0[qc] = flip(d1[t], rng.permutation(480)[:m])
        d0[lone_q] = flip(d1[n1 - 1], rng.permutation(480)[:30])
        case = Case(f"seed{v}", d0, [d1], ((BIG, RATIO_HALF), (BIG, 1.5), (150, RATIO_HALF), (150, 1.5)))
        dist = M.distances(d1, d0)                                       # the opposite direction: train rows as queries
        for t, qa, qb, qc, kind in plan:
            m = int(dist[t, qa])
            assert 1 <= m <= MAX_M and dist[t, qb] == second_bits(kind, m) and (qc is None or dist[t, qc] == m)
            assert np.delete(dist[t], [q for q in (qa, qb, qc) if q is not None]).min() > FAR_FROM
        assert dist[n1 - 1, lone_q] == 30 and np.delete(dist[n1 - 1], lone_q).min() >= 150
        rev = M.descriptor_match(d1, d0, BIG, 1.5)
        name = dict(zip(rev["index_0"].tolist(), rev["index_1"].tolist()))
        for t, qa, qb, qc, kind in plan:                                 # the lowest query index among equal minima
            assert name[t] == (min(q for q in (qa, qb, qc) if q is not None) if kind == "tie" else qa)
        out.append((case, plan))
    sides = {(qa < seed_rows, qb < seed_rows, kind) for _, plan in out for _, qa, qb, _, kind in plan}
    for kind in ("4m", "4m+1", "tie"):
        assert {(True, False, kind), (False, True, kind), (False, False, kind), (True, True, kind)} <= sides, kind
    return out


def all_cases(g):
    """{name: Case} of every case; the planted and seed-boundary plans ride along in a second dict"""
    cases, plans = {}, {}
    for n0 in (33, 513):
        case, plan = planted(g, n0)
        cases[case.name], plans[case.name] = case, plan
    for build in (lone, far, tail_bits, padded64):
        case = build(g)
        cases[case.name] = case
    case = far(g, 513)
    cases[case.name] = case
    for case, plan in seed_boundary(g):
        cases[case.name], plans[case.name] = case, plan
    return cases, plans
