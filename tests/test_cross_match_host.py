"""Cross-checked matching on the host (akz_descriptor_match_cross_host; no GPU call): the list against the oracle's
descriptor_match called in both directions and intersected in Python, on planted descriptor sets in which every way a forward
match can lose its cross-check occurs; the refusals; the declarations; and what the seeded composite promises over that list.

The planted sets (planted_sets): B is random base rows -- random 486-bit rows lie about 243 bits apart and never pass a ratio
test --, A is copies of base rows with a chosen number of flipped bits, shuffled:
  mutual         one copy at 0..8 bits                        kept
  rival          two copies of one base row, 3 and 30 bits    both pass forward, only the 3-bit one is kept
  reverse-ratio  two copies at 10 and 11 bits                 both pass forward; 10 < 11 * 0.86^2 fails: neither is kept at 0.86
  tie            two copies at 5 bits each, different bits    dropped at 0.86 (5 < 5 * 0.74 fails), at 2.0 the lower index is kept
  orphan         a base row without a copy                    nothing names it (below ratio 1)
  stranger       a query row unrelated to B                   passes in neither direction (below ratio 1)
A set needs 7 query rows and 4 base rows before it can hold one of each copied kind: the sizes 0, 1 and 7 of the size sweep are
prefixes of a full set and are held to the oracle only; the full sets are also held to `0 < len(cross) < len(fwd)` and to the
table above."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_match_pairs_host import ROOT
from test_seeded_ransac_host import options, same4

NEW_SYMBOLS = ("akz_descriptor_match_cross_host", "akz_descriptor_match_cross", "akz_descriptor_match_cross_device",
               "akz_match_features_seeded_cross_pairs")
KINDS = ("mutual", "rival", "reverse-ratio", "tie", "orphan", "stranger")


def _flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def planted_sets(seed, nb=61, mutual=40, rival=6, reverse_ratio=6, tie=6, orphan=8, stranger=20, shuffle=True):
    """-> (A, B, kind_a, base_a, kind_b): A's rows with their kind and base row (-1: a stranger), B's rows with the kind of their
    copies ("orphan": none).  Bits are flipped among the first 480, so rows of 61 and of 64 bytes are built alike."""
    rng = np.random.default_rng(seed)
    n_b = mutual + rival + reverse_ratio + tie + orphan
    B = rng.integers(0, 256, (n_b, nb), dtype=np.uint8)
    kind_b = ["mutual"] * mutual + ["rival"] * rival + ["reverse-ratio"] * reverse_ratio + ["tie"] * tie + ["orphan"] * orphan
    order_b = rng.permutation(n_b) if shuffle else np.arange(n_b)
    B, kind_b = B[order_b], [kind_b[i] for i in order_b]
    rows, kind_a, base_a = [], [], []
    for j, kind in enumerate(kind_b):
        bits = rng.permutation(480)
        if kind == "mutual":
            flips = [bits[:int(rng.integers(0, 9))]]
        elif kind == "rival":
            flips = [bits[:3], bits[3:33]]
        elif kind == "reverse-ratio":
            flips = [bits[:10], bits[10:21]]
        elif kind == "tie":
            flips = [bits[:5], bits[5:10]]
        else:
            flips = []
        for f in flips:
            rows.append(_flip(B[j], f))
            kind_a.append(kind)
            base_a.append(j)
    for _ in range(stranger):
        rows.append(rng.integers(0, 256, nb, dtype=np.uint8))
        kind_a.append("stranger")
        base_a.append(-1)
    A = np.array(rows, np.uint8).reshape(len(rows), nb)
    order_a = rng.permutation(len(A)) if shuffle else np.arange(len(A))
    return A[order_a], B, [kind_a[i] for i in order_a], np.array([base_a[i] for i in order_a], np.int64), kind_b


def oracle_cross(ref, a, b, thr, ratio):
    """-> (cross, fwd, rev): the oracle's descriptor_match in both directions, intersected here"""
    nb = a.shape[1]
    if len(a) == 0 or len(b) == 0:
        empty = np.zeros(0, ref.MATCH_DTYPE)
        fwd = ref.descriptor_match(a, b, thr, ratio) if len(a) else empty
        return empty, fwd, empty
    fwd = ref.descriptor_match(a.reshape(-1, nb), b.reshape(-1, nb), thr, ratio)
    rev = ref.descriptor_match(b.reshape(-1, nb), a.reshape(-1, nb), thr, ratio)
    back = {int(r["index_0"]): int(r["index_1"]) for r in rev}
    keep = [k for k, m in enumerate(fwd) if back.get(int(m["index_1"])) == int(m["index_0"])]
    return fwd[keep], fwd, rev


def check_kinds(cross, fwd, kind_a, base_a, kind_b, ratio, thr=10000):
    """the table of the module's docstring on a full set at threshold 10000: every kind occurs, and behaves as stated"""
    assert thr == 10000
    assert set(kind_a) | set(kind_b) == set(KINDS), (set(kind_a), set(kind_b))
    assert 0 < len(cross) < len(fwd)
    in_fwd, in_cross = set(fwd["index_0"].tolist()), set(cross["index_0"].tolist())
    for kind in ("mutual", "rival", "reverse-ratio", "tie"):            # every copy passes forward, and names its base row
        rows = [i for i, k in enumerate(kind_a) if k == kind]
        assert rows and all(i in in_fwd for i in rows), kind
    assert all(int(m["index_1"]) == base_a[int(m["index_0"])] for m in fwd if base_a[int(m["index_0"])] >= 0)
    if ratio < 1:      # (from ratio 1 on nearly every row passes: a stranger then finds some row, and an orphan may be it)
        assert not any(i in in_fwd for i, k in enumerate(kind_a) if k == "stranger")
        assert not any(kind_b[int(j)] == "orphan" for j in fwd["index_1"])
    dist = {int(m["index_0"]): m["distance"] for m in fwd}
    for j, kind in enumerate(kind_b):
        copies = [i for i in range(len(kind_a)) if base_a[i] == j]
        kept = [i for i in copies if i in in_cross]
        if kind == "mutual":
            assert kept == copies and len(copies) == 1
        elif kind == "rival":                                            # only the 3-bit copy
            assert len(copies) == 2 and len(kept) == 1 and dist[kept[0]] == 3.0 and sorted(dist[i] for i in copies) == [3.0, 30.0]
        elif kind == "reverse-ratio":                                    # 10 < 11 * ratio^2 ?
            assert sorted(dist[i] for i in copies) == [10.0, 11.0]
            assert [dist[i] for i in kept] == ([10.0] if 10 < 11 * ratio * ratio else [])
        elif kind == "tie":                                              # 5 < 5 * ratio^2 ?  then the lower index
            assert [dist[i] for i in copies] == [5.0, 5.0]
            assert kept == ([min(copies)] if ratio * ratio > 1 else [])


@pytest.fixture(scope="module")
def full():
    return {nb: planted_sets(1600 + nb, nb) for nb in (61, 64)}


def test_symbols_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert L.akz_abi_version() == 6
    assert C.sizeof(amd.RansacOptions) == 80
    for name in ("descriptor_match_cross_host", "match_features_seeded", "match_features_seeded_pairs"):
        assert callable(getattr(amd, name)), name
    for name in ("descriptor_match_cross", "descriptor_match_cross_device", "match_features_seeded_pairs"):
        assert callable(getattr(amd.Context, name)), name
    import inspect
    for fn in (amd.Context.match_features_seeded_pairs, amd.match_features_seeded_pairs, amd.match_features_seeded):
        assert inspect.signature(fn).parameters["cross_check"].default is False


@pytest.mark.parametrize("nb", [61, 64])
def test_full_sets_equal_the_oracle_intersection(amd, ref, full, nb):
    a, b, kind_a, base_a, kind_b = full[nb]
    cut = 0
    for ratio in (0.86, 1.0, 2.0):
        for thr in (10000, 8):                        # 8 cuts the 8-bit mutual copies and everything beyond
            exp, fwd, rev = oracle_cross(ref, a, b, thr, ratio)
            got = amd.descriptor_match_cross_host(a, b, thr, ratio)
            assert got.dtype == exp.dtype and np.array_equal(got, exp), (nb, ratio, thr, len(got), len(exp))
            if thr == 10000:
                check_kinds(got, fwd, kind_a, base_a, kind_b, ratio)
                full_fwd = len(fwd)
            else:
                assert 0 < len(fwd) < full_fwd and 0 < len(got)
                cut += 1
    assert cut == 3


def test_sizes_crossed(amd, ref, full):
    """n0, n1 in {0, 1, 7, 300} crossed.  The 300 x 300 case holds every kind and is held to `0 < len(cross) < len(fwd)` itself;
    a set of 0, 1 or 7 rows cannot hold one of each kind (module docstring), so those cases are prefixes, held to the oracle."""
    a, b = full[61][:2]
    big_a, big_b, kind_a, _, kind_b = planted_sets(77, 61, mutual=200, rival=10, reverse_ratio=10, tie=10, orphan=10, stranger=40)
    assert len(big_a) == 300 and len(big_b) == 240 and set(kind_a) | set(kind_b) == set(KINDS)
    dropped = 0
    for n0 in (0, 1, 7, 300):
        for n1 in (0, 1, 7, 300):
            x = (big_a if n0 == 300 else a)[:n0]
            y = (np.concatenate([big_b, big_a[:60]]) if n1 == 300 else b)[:n1]        # (300: the 240 base rows and 60 rows of A itself)
            assert (len(x), len(y)) == (n0, n1)
            for ratio in (0.86, 2.0):
                exp, fwd, _ = oracle_cross(ref, x, y, 10000, ratio)
                got = amd.descriptor_match_cross_host(x, y, 10000, ratio)
                assert np.array_equal(got, exp), (n0, n1, ratio)
                if (n0, n1) == (300, 300):
                    assert 0 < len(got) < len(fwd), (ratio, len(got), len(fwd))
                dropped += len(fwd) - len(got)
    assert dropped > 0


@pytest.mark.parametrize("nb", [61, 64])
def test_a_set_against_itself(amd, ref, full, nb):
    """cross(A, A).  Both directions are the same scan, so the reverse list IS the forward list: a record i -> i points back at
    itself, and no record i -> j with j != i can pass -- j would be an exact duplicate of i at distance 0, and then the second
    best, i itself, is 0 too.  So cross(A, A) == descriptor_match(A, A) by the statement, and the strict `len(cross) < len(fwd)`
    that the other tests assert cannot hold here; what is dropped from BOTH lists is the duplicated rows, which this input has."""
    a, _, kind_a, _, kind_b = full[nb]
    assert set(kind_a) | set(kind_b) == set(KINDS)
    a = np.concatenate([a, a[:5]])                    # five exact duplicates: their ratio test fails in both directions
    for ratio in (0.86, 2.0):
        exp, fwd, _ = oracle_cross(ref, a, a, 10000, ratio)
        got = amd.descriptor_match_cross_host(a, a, 10000, ratio)
        assert np.array_equal(got, exp) and np.array_equal(got, fwd)
        assert 0 < len(got) == len(a) - 10 and np.array_equal(got["index_0"], got["index_1"])


def test_refusals(amd, full):
    a, b = full[61][:2]
    L = amd.lib()
    out = np.zeros(len(a), amd.MATCH_DTYPE)
    out["index_0"] = 77
    n = C.c_uint64(12345)
    pa, pb, po = a.ctypes.data, b.ctypes.data, out.ctypes.data
    for k, args in enumerate(((None, len(a), pb, len(b), 61, 10000, 0.86, po, C.byref(n)),
                              (pa, len(a), None, len(b), 61, 10000, 0.86, po, C.byref(n)),
                              (pa, len(a), pb, len(b), 61, 10000, 0.86, None, C.byref(n)),
                              (pa, len(a), pb, len(b), 61, 10000, 0.86, po, None),
                              (pa, len(a), pb, len(b), 0, 10000, 0.86, po, C.byref(n)),
                              (pa, len(a), pb, len(b), 65, 10000, 0.86, po, C.byref(n)))):
        assert L.akz_descriptor_match_cross_host(*args) != 0, k
        assert n.value == 12345 and np.all(out["index_0"] == 77), k
    # the pointers of an empty side may be null, as for akz_descriptor_match
    assert L.akz_descriptor_match_cross_host(None, 0, pb, len(b), 61, 10000, 0.86, None, C.byref(n)) == 0 and n.value == 0
    n.value = 5
    assert L.akz_descriptor_match_cross_host(pa, len(a), None, 0, 61, 10000, 0.86, po, C.byref(n)) == 0 and n.value == 0
    assert L.akz_descriptor_match_cross(None, pa, len(a), pb, len(b), 61, 10000, 0.86, po, C.byref(n)) != 0     # no context
    assert L.akz_descriptor_match_cross_device(None, pa, len(a), pb, len(b), 10000, 0.86, po, C.byref(n)) != 0


def cross_scene(amd, model, n, seed, nb=61):
    """a planted two-view case of the seeded tests whose first set also holds, for some of its matches, a rival (a second copy of
    the match's train row at 30 bits, with a keypoint of its own) -> (fa, fb): descriptor_match keeps the rivals, the cross-check
    drops them"""
    from test_gpu_fundamental_refit import planted_case as pf
    from test_gpu_homography_refit import planted_case as ph
    fa, fb = (pf if model == "F" else ph)(amd, n, seed, nb=nb)[:2]
    rng = np.random.default_rng(seed + 1)
    extra = max(1, n // 4)
    where = {d.tobytes(): j for j, d in enumerate(fb[1])}
    ka, da = fa[0][:len(fa[1])].copy(), fa[1].copy()
    rk, rd = np.zeros(extra, amd.KEYPOINT_DTYPE), np.zeros((extra, nb), np.uint8)
    for t in range(extra):
        j = where[da[t].tobytes()]
        rd[t] = _flip(fb[1][j], rng.permutation(480)[:30])
        rk[t] = ka[t]
        rk[t]["x"], rk[t]["y"] = rng.uniform(0, 1920), rng.uniform(0, 1080)
    return (np.concatenate([ka, rk]), np.concatenate([da, rd])), fb


@pytest.mark.parametrize("model", ["H", "F"])
def test_remove_outliers_seeded_over_the_cross_list(amd, ref, model):
    """what akz_match_features_seeded_cross_pairs promises per pair, formed on the host: the seeded RANSAC over the cross list --
    which is shorter than the forward list, holds none of the planted rivals, and gives a model"""
    fa, fb = cross_scene(amd, model, 257, 757)
    exp, fwd, _ = oracle_cross(ref, fa[1], fb[1], 10000, 0.86)
    raw = amd.descriptor_match_cross_host(fa[1], fb[1], 10000, 0.86)
    assert np.array_equal(raw, exp) and len(raw) == 257 and len(fwd) == 257 + 64
    opt = options(amd, model, max_trials=384, confidence=0.99, refine_iterations=2, epsilon_inliers=4.0 if model == "F" else 3.0)
    got = amd.remove_outliers_seeded(fa[0], fb[0], raw, opt, stream=5)
    same4(got, amd.remove_outliers_seeded(fa[0], fb[0], exp, opt, stream=5), model)
    assert got[1] is not None and 0 < len(got[0]) <= 257
    assert np.all(got[0]["index_0"] < 257) and np.any(fwd["index_0"] >= 257)         # the rivals are the rows from 257 on
