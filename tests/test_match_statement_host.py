"""The numpy statement of the matcher (tests/match_numpy.py) and its cases (tests/match_cases.py) have teeth; no GPU call.

  * the literal form (byte loop with the bail-out) equals the vectorised form, under every switch as well: the bail-out is
    invisible;
  * the statement equals the oracle's descriptor_match on every case and on a few hundred small random sets (rows of 1, 7, 61
    and 64 bytes, every threshold and ratio of the cases, ratio 0, a negative ratio, ratios above 1), and the derived
    statements equal akz_descriptor_match_cross_host, akz_descriptor_match_knn_host and akz_descriptor_match_guided_host under
    a gate that admits every row;
  * every mutation switch changes the list of at least 3 queries of the case TEETH names (a "query" of a case with several train
    sets is a (train set, query) pair: what one record of the multi-set launch answers), and no case is idle under all switches;
  * every simulated kernel fault (FAULTS: written here in numpy from the tile size, the lane map (i & 3) + 8 (i >> 2) + 4 h, the
    chunk cut and the seed rows, applied to the TRUE distance matrix) is caught by at least 3 queries of the case it names, and
    the same models without the fault give the statement's lists exactly -- the parallel forms are order-free;
  * what the inputs of tests/test_gpu_fp4_walk.py could not see, as assertions, and the settings that test now runs at.

Measured counts (T = 128, MT = 256, seed rows 2048), queries whose record changes at the setting TEETH / FAULTS name (the tests
print them and assert >= 3 of each; this table is what one run printed):
  switch                      case         count      fault                        case          count
  min_le                      planted33      132      pad_244                      far33           165
  tie_not_second              planted33       80      pad_query_weight             far33           165
  min_starts_unbounded        lone33          15      drop_last_row                planted33        10
  thr_le                      lone33           8      lane0_wins_ties              planted33        40
  ratio_le                    planted33       62      second_from_seconds (2/3/5)  planted33  37/56/66
  ratio_f32                   planted33       21      skip_equal_second            seed0             4
  ratio_unsquared             planted33       62      seed_only                    seed0             5
  bits_486                    tail33          33
  bytes_61_of_64              padded64_33     33
  second_from_seconds         planted33       34
  second_starts_unbounded     proven invisible (INVISIBLE, test_the_seconds_start_is_invisible)

One simulated fault is invisible to a sequential scan and PROVEN so here (test_skipping_a_row_at_the_second_is_invisible_in_order):
a row whose distance equals the current second changes nothing when rows arrive in ascending order -- it cannot lower the
second, and it is below the minimum only if min == second == d, which is not strictly below.  It shows only where rows arrive
out of order (the atomic candidates of the both-direction form): three rows at the minimum's distance, the lowest index last."""
import itertools

import numpy as np
import pytest

import match_cases as MC
import match_numpy as M

RATIOS = (0.0, -0.86, 0.5, MC.RATIO_SQRT_HALF, 0.86, 0.99, 1.0, 1.3, 1.5, 2.0)


@pytest.fixture(scope="module")
def world(amd):
    g = MC.geometry(amd)
    cases, plans = MC.all_cases(g)
    return g, cases, plans


def changed(a, b):
    """queries whose record differs between two lists"""
    ra = {int(r["index_0"]): (int(r["index_1"]), float(r["distance"])) for r in a}
    rb = {int(r["index_0"]): (int(r["index_1"]), float(r["distance"])) for r in b}
    return sum(ra.get(i) != rb.get(i) for i in set(ra) | set(rb))


def same(got, exp, what):
    assert got.dtype == exp.dtype and np.array_equal(got, exp), (what, len(got), len(exp))


# ---- the two forms of the statement -----------------------------------------------------------------------------------------
def small_sets(rng, nb, n0=None, n1=None):
    """random rows with copies, near copies and repeated rows: ties, zero distances and distances around any small threshold"""
    n0 = int(rng.integers(1, 9)) if n0 is None else n0
    n1 = int(rng.integers(0, 12)) if n1 is None else n1
    a = rng.integers(0, 256, (n0, nb), dtype=np.uint8)
    b = rng.integers(0, 256, (n1, nb), dtype=np.uint8)
    for j in range(n1):
        if rng.random() < 0.6:
            b[j] = MC.flip(a[rng.integers(0, n0)], rng.integers(0, 8 * nb, rng.integers(0, 6)))
    return a, b


def test_literal_form_equals_vectorised_form():
    rng = np.random.default_rng(11)
    n = 0
    for nb in (1, 7, 61, 64):
        for _ in range(12):
            a, b = small_sets(rng, nb)
            dist = M.distances(a, b)
            assert np.array_equal(dist, M.distances_unpackbits(a, b))
            assert np.array_equal(M.distances(a, b, ("bits_486", "bytes_61_of_64")), M.distances_unpackbits(a, b, ("bits_486", "bytes_61_of_64")))
            for thr, ratio in itertools.product((0, 1, 3, 4 * nb, 10000, 2 ** 31, 2 ** 63 - 1), (0.0, -0.86, 0.5, 1.0, 1.5)):
                vec = M.descriptor_match(a, b, thr, ratio)
                same(M.descriptor_match(a, b, thr, ratio, form="literal"), vec, (nb, thr, ratio))
                n += 1
            for switch in M.SWITCHES:                                   # the bail-out stays invisible under every switch
                same(M.descriptor_match(a, b, 4 * nb, 1.5, (switch,), form="literal"), M.descriptor_match(a, b, 4 * nb, 1.5, (switch,)), switch)
    assert n >= 1000


def test_thresholds_above_2_31_count_as_that_value():
    rng = np.random.default_rng(12)
    a, b = small_sets(rng, 61, 8, 11)
    for ratio in (0.5, 1.0, 1.5):
        exp = M.descriptor_match(a, b, 2 ** 31 - 1, ratio)
        for thr in (2 ** 31, 2 ** 40, 2 ** 63 - 1):
            same(M.descriptor_match(a, b, thr, ratio), exp, (thr, ratio))
    assert M.ratio_squared(MC.RATIO_SQRT_HALF) == 0.5000000000000001 and M.ratio_squared(MC.RATIO_SQRT_HALF, ("ratio_f32",)) < 0.5
    assert M.ratio_squared(0.86) == 0.7395999999999999


# ---- statement against the oracle and the host forms ----------------------------------------------------------------------
def test_statement_equals_the_oracle_on_every_case(world, ref):
    g, cases, _ = world
    for case in cases.values():
        for d1 in case.sets:
            for (thr, ratio), got in M.match_settings(M.distances(case.d0, d1), case.settings).items():
                same(got, ref.descriptor_match(case.d0, d1, thr, ratio), (case.name, len(d1), thr, ratio))
        if case.name.startswith("seed"):                                # the opposite direction
            for (thr, ratio), got in M.match_settings(M.distances(case.sets[0], case.d0), case.settings).items():
                same(got, ref.descriptor_match(case.sets[0], case.d0, thr, ratio), (case.name, "reverse", thr, ratio))


def test_statement_equals_the_oracle_on_small_random_sets(ref):
    rng = np.random.default_rng(13)
    sets = 0
    for nb in (1, 7, 61, 64):
        for _ in range(60):
            a, b = small_sets(rng, nb)
            if len(b) == 0:
                b = np.zeros((0, nb), np.uint8)
            settings = list(itertools.product(MC.THRESHOLDS + (2, 3, 4 * nb, MC.LONE_M0 * 4), RATIOS))
            for (thr, ratio), got in M.match_settings(M.distances(a, b), settings).items():
                same(got, ref.descriptor_match(a, b, thr, ratio), (nb, thr, ratio))
            sets += 1
    assert sets >= 200


def one_point(amd, n):
    k = np.zeros(n, amd.KEYPOINT_DTYPE)
    k["x"], k["y"] = 10.0, 20.0
    return k


def test_derived_statements_equal_the_host_forms(world, amd):
    g, cases, _ = world
    for name in ("planted33", "lone33", "far33", "tail33", "padded64_33", "seed0"):
        case = cases[name]
        for d1 in case.sets[:5]:
            a = case.d0 if len(case.d0) <= 513 else case.d0[g.seed_tiles * g.T - 40:g.seed_tiles * g.T + 40]
            for thr, ratio in case.settings[:6]:
                same(amd.descriptor_match_cross_host(a, d1, thr, ratio), M.descriptor_match_cross(a, d1, thr, ratio), (name, "cross", thr, ratio))
                got = amd.descriptor_match_guided_host(one_point(amd, len(a)), a, one_point(amd, len(d1)), d1, np.eye(3), 0, 1.0, thr, ratio)
                same(got, M.scan_admitted(a, d1, np.ones((len(a), len(d1)), bool), thr, ratio), (name, "guided", thr, ratio))
            dist = M.distances(a, d1)
            for k, thr in itertools.product((1, 2, 8), (489, MC.BIG, 4 * MC.LONE_M0)):
                got, exp = amd.descriptor_match_knn_host(a, d1, k, thr), M.knn(a, d1, k, thr, dist)
                assert np.array_equal(got[1], exp[1]) and got[0].tobytes() == exp[0].tobytes(), (name, "knn", k, thr)
    # k = 8 against three rows: three entries and five empty slots
    far = cases["far33"]
    out, counts = M.knn(far.d0, far.sets[1], 8, MC.BIG)
    assert np.all(counts == 3) and np.all(out["index_1"][:, 3:] == M.NO_ROW) and np.all(np.isposinf(out["distance"][:, 3:]))
    # the admitted subset is a scan of its own: a row outside it neither wins nor lowers the second
    case = cases["planted33"]
    d1 = case.sets[0]
    odd = np.zeros((len(case.d0), len(d1)), bool)
    odd[:, 1::2] = True
    sub = M.scan_admitted(case.d0, d1, odd, MC.BIG, 1.5)
    exp = M.descriptor_match(case.d0, d1[1::2], MC.BIG, 1.5)
    exp["index_1"] = 2 * exp["index_1"] + 1
    same(sub, exp, "admitted subset")


# ---- every switch is caught -------------------------------------------------------------------------------------------------
# switch -> (case, (threshold, ratio), form): form "host" = every byte counts (64-byte rows through the host entry points)
TEETH = {
    "min_le": ("planted33", (MC.BIG, 1.5)),
    "tie_not_second": ("planted33", (MC.BIG, MC.RATIO_SQRT_HALF)),
    "min_starts_unbounded": ("lone33", (4 * MC.LONE_M0, 0.5)),
    "thr_le": ("lone33", (4 * MC.LONE_M0, 1.5)),
    "ratio_le": ("planted33", (MC.BIG, 0.5)),
    "ratio_f32": ("planted33", (MC.BIG, MC.RATIO_SQRT_HALF)),
    "ratio_unsquared": ("planted33", (MC.BIG, 0.5)),
    "bits_486": ("tail33", (MC.BIG, 1.5)),
    "bytes_61_of_64": ("padded64_33", (MC.BIG, 1.5)),
    "second_from_seconds": ("planted33", (MC.BIG, 0.5)),
}


# Proven invisible (test_the_seconds_start_is_invisible): the second's start never reaches a record.  While no row is below the
# threshold the minimum stays AT the threshold and the query fails min < threshold whatever the second holds.  The first row below
# the threshold finds the minimum still at the threshold and hands exactly that to the second (:44), overwriting whatever the second
# held -- from there on the state is the true one.  (The MINIMUM's start is visible: started unbounded, the first row hands
# "unbounded" on, and a lone row below the threshold meets a second above it.)
INVISIBLE = ("second_starts_unbounded",)


def switch_count(case, setting, mut):
    thr, ratio = setting
    return sum(changed(M.descriptor_match(case.d0, d1, thr, ratio, mut), M.descriptor_match(case.d0, d1, thr, ratio)) for d1 in case.sets)


def test_every_switch_is_caught(world):
    _, cases, _ = world
    assert set(TEETH) == set(M.SWITCHES) - set(INVISIBLE)
    seen = {}
    for switch, (name, setting) in TEETH.items():
        seen[switch] = switch_count(cases[name], setting, (switch,))
        print(f"switch {switch:26s} {name:12s} {setting} {seen[switch]}")
    assert all(n >= 3 for n in seen.values()), seen


def test_the_seconds_start_is_invisible(world):
    """INVISIBLE, checked where the argument says it must hold: every case at every setting, and small sets at thresholds in
    the middle of their distances (rows on both sides of the threshold, in every order)"""
    _, cases, _ = world
    for case in cases.values():
        for d1 in case.sets[:4]:
            dist = M.distances(case.d0, d1)
            exp = M.match_settings(dist, case.settings)
            for setting, got in M.match_settings(dist, case.settings, INVISIBLE).items():
                same(got, exp[setting], (case.name, setting))
    rng = np.random.default_rng(14)
    for _ in range(100):
        a, b = small_sets(rng, 7)
        dist = M.distances(a, b)
        settings = list(itertools.product(range(0, 40, 3), (0.5, 1.0, 1.5)))
        exp = M.match_settings(dist, settings)
        for setting, got in M.match_settings(dist, settings, INVISIBLE).items():
            same(got, exp[setting], setting)
        for state, true in zip(M.top2(dist, 12, INVISIBLE), M.top2(dist, 12)):      # the STATE differs only where min == threshold
            assert np.array_equal(state[M.top2(dist, 12)[0] < 12], true[M.top2(dist, 12)[0] < 12])


def test_no_case_is_idle_under_all_switches(world):
    _, cases, _ = world
    for case in cases.values():
        d0 = case.d0 if len(case.d0) <= 513 else case.d0[-600:]
        hit = set()
        for d1 in case.sets[:1] + case.sets[-1:]:
            true_dist = M.distances(d0, d1)
            exp = M.match_settings(true_dist, case.settings[:6])
            for s in M.SWITCHES:
                dist = M.distances(d0, d1, (s,)) if s in ("bits_486", "bytes_61_of_64") else true_dist
                got = M.match_settings(dist, case.settings[:6], (s,))
                if any(changed(got[k], exp[k]) for k in exp):
                    hit.add(s)
        assert hit, case.name
        print(f"case {case.name:12s} moved by {sorted(hit)}")


# ---- simulated kernel faults --------------------------------------------------------------------------------------------------
def feed(state, d, j):
    """top2_feed of the kernels on arrays: (min, second, argmin) <- a candidate (d, j)"""
    mn, second, mj = state
    new = d < mn
    lower = ~new & (d < second)
    return np.where(new, d, mn), np.where(new, mn, np.where(lower, d, second)), np.where(new, j, mj)


def tiled_lists(g, d0, d1, thr, ratio, chunks=1, fault=None):
    mn, second, mj = tiled_state(g, d0, d1, thr, chunks, fault)
    return M.records(M.accept(mn, second, thr, ratio), mn, mj)


def tiled_state(g, d0, d1, thr, chunks=1, fault=None, dist=None):
    """The matrix-core scan as its kernels cut it, on the true distance matrix: chunks of ceil(tiles / chunks) tiles; in a
    chunk the two half-lanes of a column scan their rows (ascending) apart and are merged (the lower minimum, the lower row
    among equal minima; second = min of the seconds and the losing minimum); the chunk records are folded in ascending order
    (top2_feed on the minima, then second = min(second, the chunk's second)).  fault: one of FAULTS' names."""
    thr = M.clamp_threshold(thr)
    dist = M.distances(d0, d1) if dist is None else dist
    n0, n1 = dist.shape
    if fault == "drop_last_row":
        dist, n1 = dist[:, :-1], n1 - 1
    rows = np.arange(n1)
    pad = (-n1) % g.T
    if fault in ("pad_244", "pad_query_weight") and pad:                 # the padding rows of the last tile take part
        weight = np.unpackbits(d0, axis=1).sum(1).astype(np.int64) if fault == "pad_query_weight" else np.full(n0, 244, np.int64)
        dist = np.concatenate([dist, np.repeat(weight[:, None], pad, axis=1)], axis=1)
        rows = np.arange(n1 + pad)
    tiles = max(1, -(-n1 // g.T))
    per = -(-tiles // max(1, min(chunks, tiles)))
    state = (np.full(n0, thr, np.int64), np.full(n0, thr, np.int64), np.zeros(n0, np.int64))
    for c in range(-(-tiles // per)):
        mine = rows[(rows // g.T) // per == c]
        lanes = []
        for h in (0, 1):
            cols = mine[MC.lane_half(mine) == h]
            mn, second, mj = M.top2(dist[:, cols], thr)
            lanes.append((mn, second, np.where(mn < thr, cols[np.minimum(mj, max(len(cols) - 1, 0))] if len(cols) else 0, 0)))
        (m0, s0, j0), (m1, s1, j1) = lanes
        if fault == "lane0_wins_ties":
            other = m1 < m0
        else:
            other = (m1 < m0) | ((m1 == m0) & (m1 < thr) & (j1 < j0))
        rec = (np.where(other, m1, m0), np.where(other, np.minimum(s1, m0), np.minimum(s0, m1)), np.where(other, j1, j0))
        if fault == "second_from_seconds":                               # the losing chunk's minimum is forgotten
            new = rec[0] < state[0]
            state = (np.where(new, rec[0], state[0]), np.minimum(state[1], rec[1]), np.where(new, rec[2], state[2]))
        else:
            state = feed(state, rec[0], rec[2])
            state = (state[0], np.minimum(state[1], rec[1]), state[2])
    return state


def mutual_lists(g, d0, d1, thr, ratio, fault=None, order="descending"):
    """The opposite direction of the both-direction form: every train row's exact top-2 over the first seed rows of the query
    set, then the queries beyond the seed one by one, in `order`, through the packed exchange
        old = min-exchange(cbest, d << 32 | q);  csecond = min(csecond, max(old, mine) >> 32)
    where a candidate above the row's csecond (or not below the threshold) is skipped."""
    thr = M.clamp_threshold(thr)
    dist = M.distances(d1, d0)                                           # train rows as queries
    seed = min(len(d0), g.seed_tiles * g.T)
    mn, second, mj = M.top2(dist[:, :seed], thr)
    best = mn * (1 << 32) + np.where(mn < thr, mj, 0)
    if fault != "seed_only":
        later = range(seed, len(d0))
        for q in (reversed(later) if order == "descending" else later):
            d = dist[:, q]
            enters = (d < thr) & ((d < second) if fault == "skip_equal_second" else (d <= second))
            mine = d * (1 << 32) + q
            loser = np.maximum(best, mine) >> 32
            best = np.where(enters, np.minimum(best, mine), best)
            second = np.where(enters & (loser < thr), np.minimum(second, loser), second)
    mn, mj = best >> 32, best & 0xFFFFFFFF
    return M.records(M.accept(mn, second, thr, ratio), mn, mj)


# fault -> (case, (threshold, ratio), forced chunk counts it is applied under)
FAULTS = {
    "pad_244": ("far33", (MC.BIG, 1.5), (1,)),
    "pad_query_weight": ("far33", (MC.BIG, 1.5), (1,)),
    "drop_last_row": ("planted33", (MC.BIG, 1.5), (1,)),
    "lane0_wins_ties": ("planted33", (MC.BIG, 1.5), (1,)),
    "second_from_seconds": ("planted33", (MC.BIG, 0.5), (2, 3, 5)),
    "skip_equal_second": ("seed0", (MC.BIG, 1.5), (1,)),
    "seed_only": ("seed0", (MC.BIG, 0.5), (1,)),
}


def fault_count(g, case, setting, fault, chunks):
    thr, ratio = setting
    if fault in ("skip_equal_second", "seed_only"):
        return sum(changed(mutual_lists(g, case.d0, d1, thr, ratio, fault), M.descriptor_match_reverse(case.d0, d1, thr, ratio)) for d1 in case.sets)
    return sum(changed(tiled_lists(g, case.d0, d1, thr, ratio, chunks, fault), M.descriptor_match(case.d0, d1, thr, ratio)) for d1 in case.sets)


def test_the_parallel_forms_are_order_free(world):
    """the models above WITHOUT a fault give the statement's lists on every case: what a fault changes is the fault's doing"""
    g, cases, _ = world
    for case in cases.values():
        if case.d0.shape[1] != 61:
            continue
        for d1 in case.sets[:3] + case.sets[-1:]:
            if case.name.startswith("seed"):
                for thr, ratio in case.settings[1:3]:
                    exp = M.descriptor_match_reverse(case.d0, d1, thr, ratio)
                    for order in ("ascending", "descending"):
                        same(mutual_lists(g, case.d0, d1, thr, ratio, None, order), exp, (case.name, order, thr, ratio))
                continue
            dist = M.distances(case.d0, d1)
            for thr in sorted({thr for thr, _ in case.settings})[:3]:
                exp = M.top2(dist, thr)
                for chunks in MC.CHUNKS:                                 # the whole state, which every ratio is then tested on
                    for got, want, what in zip(tiled_state(g, case.d0, d1, thr, chunks, None, dist), exp, ("min", "second", "argmin")):
                        live = exp[0] < M.clamp_threshold(thr) if what == "argmin" else slice(None)
                        assert np.array_equal(got[live], want[live]), (case.name, len(d1), chunks, thr, what)


def test_every_simulated_fault_is_caught(world):
    g, cases, _ = world
    seen = {}
    for fault, (name, setting, chunk_counts) in FAULTS.items():
        for chunks in chunk_counts:
            seen[(fault, chunks)] = fault_count(g, cases[name], setting, fault, chunks)
            print(f"fault {fault:22s} chunks {chunks} {name:12s} {setting} {seen[(fault, chunks)]}")
    assert all(n >= 3 for n in seen.values()), seen
    # a padding row that takes part changes every query of the far case: each one's nearest real row is at 408 bits or more
    assert seen[("pad_244", 1)] >= len(cases["far33"].d0) and seen[("pad_query_weight", 1)] >= len(cases["far33"].d0)


def test_skipping_a_row_at_the_second_is_invisible_in_order(world):
    """In ascending order a row with d == second changes nothing (module docstring): skipping it gives the same state on
    every case, ties and triple ties included; out of order it is the fault FAULTS names."""
    g, cases, _ = world
    for case in cases.values():
        for d1 in case.sets[:3]:
            dist = M.distances(case.d0, d1) if not case.name.startswith("seed") else M.distances(d1, case.d0)
            for thr in (MC.BIG, 4 * MC.LONE_M0, 150):
                state = tuple(np.full(len(dist), thr, np.int64) for _ in range(2)) + (np.zeros(len(dist), np.int64),)
                for j in range(dist.shape[1]):
                    d = dist[:, j]
                    fed = feed(state, d, j)
                    state = tuple(np.where(d == state[1], old, new) for old, new in zip(state, fed))
                for got, exp in zip(state, M.top2(dist, thr)):
                    assert np.array_equal(got, exp), (case.name, thr)
    seed = cases["seed0"]
    assert changed(mutual_lists(g, seed.d0, seed.sets[0], MC.BIG, 1.5, "skip_equal_second", "ascending"),
                   M.descriptor_match_reverse(seed.d0, seed.sets[0], MC.BIG, 1.5)) == 0


# ---- what the FP4 walk test's inputs could not see ---------------------------------------------------------------------------
def test_the_walk_tests_inputs_and_settings(world):
    import test_gpu_fp4_walk as W
    g, _, _ = world
    d0, d1 = W.sets(33, 2 * g.T + 1)
    # its former second setting compared empty lists
    assert len(M.descriptor_match(d0, d1, 12, 0.99)) == 0
    assert all(len(M.descriptor_match(*W.sets(33, n1), 12, 0.99)) == 0 for n1 in W.train_sizes(g.T))
    assert len(M.descriptor_match(*W.sets(513, 5 * g.T + 1), 12, 0.99)) == 0
    mn, second, _ = M.top2(M.distances(d0, d1), 12)
    assert np.array_equal(mn, second)                                    # min == second for every query
    # and none of these faults moves one of its records
    for ratio, thr in ((1.5, 10000), (0.99, 12)):
        exp = M.descriptor_match(d0, d1, thr, ratio)
        for fault, chunks in (("pad_244", 1), ("pad_query_weight", 1), ("drop_last_row", 1), ("second_from_seconds", 2),
                              ("second_from_seconds", 3), ("second_from_seconds", 5)):
            assert changed(tiled_lists(g, d0, d1, thr, ratio, chunks, fault), exp) == 0, (fault, chunks, ratio, thr)
        assert changed(M.descriptor_match(d0, d1, thr, ratio, ("bits_486",)), exp) == 0
    # the settings it runs at now: every list non-empty and shorter than n0, on every case
    assert (0.99, 12) not in W.TOP2 and len(W.TOP2) >= 2
    for n0 in W.N0:
        for n1 in W.train_sizes(g.T):
            a, b = W.sets(n0, n1)
            for ratio, thr in W.TOP2:
                assert 0 < len(M.descriptor_match(a, b, thr, ratio)) < n0, (n0, n1, ratio, thr)
