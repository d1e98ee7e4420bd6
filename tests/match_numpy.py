"""The descriptor matcher as a numpy statement, written from akaze/src/ops/feature_matching.rs:23-123 and the words of
include/akaze_hip.h alone: it imports neither the oracle nor the product, and is the second witness of every
matching kernel and host form.

  descriptor_match(d0, d1, threshold, ratio, mut=(), form=...)   the list of feature_matching.rs:23-94
      form "literal": the byte loop with the bail-out of :113-123, one Python step per byte, for small sets;
      form "vector":  a distance matrix (np.unpackbits of the XOR, summed; np.bitwise_count on 64-bit words where numpy has it),
                      then the same sequential rule row by row (column after column, every query at once), for the larger ones.
  top2 / accept / records   the three steps of the vectorised form, apart: a simulated kernel fault (tests/
                      test_match_statement_host.py) changes the distance matrix or the (min, second, argmin) state and goes
                      through the same acceptance.
  descriptor_match_reverse, descriptor_match_cross, knn, scan_admitted   what the header derives from the one scan.

The rule: both distances start at the threshold (:38-40); a row strictly below the minimum takes it and hands the old minimum
to the second (:43-46), otherwise a row strictly below the second lowers it (:47-49) -- so the lowest index wins among equal
minima and an equal distance lowers the second; a query is kept iff (min as f64) < (second as f64) * ratio * ratio (:61, ratio
squared as a product of Python floats) and min < threshold (:62).  Thresholds above 2^31 - 1 count as that value
(include/akaze_hip.h).

Mutation switches (`mut`, a collection of names): each flips ONE rule, and tests/test_match_statement_host.py shows for each a
case in which it changes the list."""
import numpy as np

MATCH_DTYPE = np.dtype([("index_0", "<u8"), ("index_1", "<u8"), ("distance", "<f8")])
THRESHOLD_MAX = 2 ** 31 - 1
UNBOUNDED = 2 ** 62                      # "above every distance"
NO_ROW = np.uint64(0xFFFFFFFFFFFFFFFF)

SWITCHES = {
    "min_le": "a later equal row replaces the minimum (:43 with <=)",
    "tie_not_second": "a row equal to the minimum does not lower the second (:47 only for rows above the minimum)",
    "second_starts_unbounded": "the second starts above every distance instead of at the threshold (:40) -- invisible, see the host test",
    "min_starts_unbounded": "the minimum starts above every distance (:38; the second still at the threshold)",
    "thr_le": "<= against the threshold (:62)",
    "ratio_le": "<= in the ratio test (:61)",
    "ratio_f32": "ratio * ratio formed in float32",
    "ratio_unsquared": "the ratio is not squared",
    "bits_486": "bits 486 and 487 (the two high bits of byte 60) are ignored",
    "bytes_61_of_64": "on 64-byte rows only the first 61 bytes count (the device entry points' contract, a fault on the host ones)",
    "second_from_seconds": "the old minimum is not handed to the second when a new minimum arrives (:44 dropped)",
}


def _check(mut):
    mut = frozenset(mut)
    assert mut <= set(SWITCHES), sorted(mut - set(SWITCHES))
    return mut


def clamp_threshold(threshold):
    return min(int(threshold), THRESHOLD_MAX)


def counted(d, mut=()):
    """the bytes of the rows that take part, with the bits a switch drops cleared"""
    mut = _check(mut)
    d = np.ascontiguousarray(d, np.uint8)
    if "bytes_61_of_64" in mut and d.shape[1] == 64:
        d = d[:, :61]
    if "bits_486" in mut and d.shape[1] >= 61:
        d = d.copy()
        d[:, 60] &= 0x3F
    return d


def distances_unpackbits(a, b, mut=()):
    """(n0, n1) hamming distances over every byte of the rows, int64: np.unpackbits of the XOR, summed"""
    a, b = counted(a, mut), counted(b, mut)
    out = np.zeros((len(a), len(b)), np.int64)
    for i in range(len(a) if len(b) else 0):
        out[i] = np.unpackbits(a[i][None, :] ^ b, axis=1).sum(axis=1, dtype=np.int64)
    return out


def distances(a, b, mut=()):
    """the same matrix for the larger sets: the rows as 64-bit words, np.bitwise_count of the XOR (numpy >= 2; held to
    distances_unpackbits by the host test)"""
    if not hasattr(np, "bitwise_count"):
        return distances_unpackbits(a, b, mut)
    a, b = counted(a, mut), counted(b, mut)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), np.int64)
    words = -(-a.shape[1] // 8)
    pa, pb = np.zeros((len(a), 8 * words), np.uint8), np.zeros((len(b), 8 * words), np.uint8)
    pa[:, :a.shape[1]], pb[:, :b.shape[1]] = a, b
    pa, pb = pa.view(np.uint64), pb.view(np.uint64)
    out = np.empty((len(a), len(b)), np.int64)
    for i in range(0, len(a), 256):
        out[i:i + 256] = np.bitwise_count(pa[i:i + 256, None, :] ^ pb[None, :, :]).sum(axis=2, dtype=np.int64)
    return out


# ---- the sequential rule ----------------------------------------------------------------------------------------------------
def top2(dist, threshold, mut=(), admitted=None):
    """feature_matching.rs:38-50 on a distance matrix: column after column, for every query at once -> (min, second, argmin),
    int64 arrays.  admitted (optional, bool (n0, n1)): rows that are not admitted are skipped (`continue`)."""
    mut = _check(mut)
    thr = clamp_threshold(threshold)
    n0, n1 = dist.shape
    mn = np.full(n0, UNBOUNDED if "min_starts_unbounded" in mut else thr, np.int64)
    second = np.full(n0, UNBOUNDED if "second_starts_unbounded" in mut else thr, np.int64)
    mj = np.zeros(n0, np.int64)
    for j in range(n1):
        d = dist[:, j]
        ok = np.ones(n0, bool) if admitted is None else admitted[:, j]
        new_min = ok & ((d <= mn) if "min_le" in mut else (d < mn))                              # :43
        lower = ok & ~new_min & (d < second)                                                       # :47
        if "tie_not_second" in mut:
            lower &= d > mn
        handed = second if "second_from_seconds" in mut else mn
        second = np.where(new_min, handed, np.where(lower, d, second))                            # :44, :48
        mj = np.where(new_min, j, mj)                                                              # :46
        mn = np.where(new_min, d, mn)                                                              # :45
    return mn, second, mj


def ratio_squared(ratio, mut=()):
    mut = _check(mut)
    if "ratio_unsquared" in mut:
        return float(ratio)
    if "ratio_f32" in mut:
        return float(np.float32(ratio) * np.float32(ratio))
    return float(ratio) * float(ratio)                                  # powi(2): one f64 product


def accept(mn, second, threshold, ratio, mut=()):
    """feature_matching.rs:61-62 -> bool per query"""
    mut = _check(mut)
    thr = clamp_threshold(threshold)
    r2 = np.float64(ratio_squared(ratio, mut))
    lhs, rhs = mn.astype(np.float64), second.astype(np.float64) * r2
    with np.errstate(invalid="ignore"):
        lowe = (lhs <= rhs) if "ratio_le" in mut else (lhs < rhs)
    return lowe & ((mn <= thr) if "thr_le" in mut else (mn < thr))


def records(keep, mn, mj):
    """the list, in index_0 order (:63-67)"""
    rows = np.flatnonzero(keep)
    out = np.zeros(len(rows), MATCH_DTYPE)
    out["index_0"], out["index_1"], out["distance"] = rows, mj[rows], mn[rows].astype(np.float64)
    return out


def match_from_distances(dist, threshold, ratio, mut=(), admitted=None):
    mn, second, mj = top2(dist, threshold, mut, admitted)
    return records(accept(mn, second, threshold, ratio, mut), mn, mj)


def match_settings(dist, settings, mut=(), admitted=None):
    """{(threshold, ratio): list} for several settings of one distance matrix (one scan per threshold)"""
    scans, out = {}, {}
    for thr, ratio in settings:
        if thr not in scans:
            scans[thr] = top2(dist, thr, mut, admitted)
        mn, second, mj = scans[thr]
        out[(thr, ratio)] = records(accept(mn, second, thr, ratio, mut), mn, mj)
    return out


def _hamming_literal(x0, x1, bailout):
    """feature_matching.rs:113-123"""
    distance = 0
    for b0, b1 in zip(x0, x1):
        distance += bin(b0 ^ b1).count("1")
        if distance > bailout:
            break
    return distance


def descriptor_match_literal(d0, d1, threshold, ratio, mut=()):
    """feature_matching.rs:23-94 as written, one Python step per byte (small sets)"""
    mut = _check(mut)
    thr = clamp_threshold(threshold)
    rows0, rows1 = [r.tolist() for r in counted(d0, mut)], [r.tolist() for r in counted(d1, mut)]
    r2 = ratio_squared(ratio, mut)
    out = []
    for i, x0 in enumerate(rows0):
        min_distance = UNBOUNDED if "min_starts_unbounded" in mut else thr
        second = UNBOUNDED if "second_starts_unbounded" in mut else thr
        min_j = 0
        for j, x1 in enumerate(rows1):
            distance = _hamming_literal(x0, x1, second)
            if distance <= min_distance if "min_le" in mut else distance < min_distance:
                if "second_from_seconds" not in mut:
                    second = min_distance
                min_distance, min_j = distance, j
            elif distance < second and not ("tie_not_second" in mut and distance == min_distance):
                second = distance
        lhs, rhs = float(min_distance), float(second) * r2
        if lhs <= rhs if "ratio_le" in mut else lhs < rhs:
            if min_distance <= thr if "thr_le" in mut else min_distance < thr:
                out.append((i, min_j, float(min_distance)))
    return np.array(out, MATCH_DTYPE) if out else np.zeros(0, MATCH_DTYPE)


def descriptor_match(d0, d1, threshold=10000, ratio=0.86, mut=(), form="vector"):
    if form == "literal":
        return descriptor_match_literal(d0, d1, threshold, ratio, mut)
    assert form == "vector"
    return match_from_distances(distances(d0, d1, mut), threshold, ratio, mut)


# ---- what the header derives from the one scan ------------------------------------------------------------------------------
def descriptor_match_reverse(d0, d1, threshold=10000, ratio=0.86, mut=()):
    """the opposite direction: the sets exchanged (index_0 a row of d1)"""
    return descriptor_match(d1, d0, threshold, ratio, mut)


def cross_filter(fwd, rev):
    """m of fwd is kept iff rev holds the record with index_0 == m.index_1 and index_1 == m.index_0 (include/akaze_hip.h)"""
    back = {int(r["index_0"]): int(r["index_1"]) for r in rev}
    keep = [k for k, m in enumerate(fwd) if back.get(int(m["index_1"])) == int(m["index_0"])]
    return fwd[keep]


def descriptor_match_cross(d0, d1, threshold=10000, ratio=0.86, mut=()):
    if len(d0) == 0 or len(d1) == 0:
        return np.zeros(0, MATCH_DTYPE)
    return cross_filter(descriptor_match(d0, d1, threshold, ratio, mut), descriptor_match_reverse(d0, d1, threshold, ratio, mut))


def knn(a, b, k, threshold=10000, dist=None):
    """for every row of a its k nearest rows of b below the threshold, ordered by (distance, index) -> (records (n0, k), counts
    (n0,) uint32); unused slots hold index_1 = 2^64 - 1 and distance = inf (include/akaze_hip.h)"""
    dist = distances(a, b) if dist is None else dist
    n0, n1 = dist.shape
    out = np.zeros((n0, k), MATCH_DTYPE)
    out["index_0"] = np.arange(n0, dtype=np.uint64)[:, None]
    out["index_1"] = NO_ROW
    out["distance"] = np.inf
    counts = np.zeros(n0, np.uint32)
    if n1 and n0:
        order = np.argsort(dist, axis=1, kind="stable")[:, :k]          # ascending distance, ascending index among equals
        near = np.take_along_axis(dist, order, axis=1)
        ok = near < clamp_threshold(threshold)                           # (ascending: the rows below the threshold come first)
        width = order.shape[1]
        counts[:] = ok.sum(axis=1)
        out["index_1"][:, :width] = np.where(ok, order.astype(np.uint64), NO_ROW)
        out["distance"][:, :width] = np.where(ok, near.astype(np.float64), np.inf)
    return out, counts


def scan_admitted(d0, d1, admitted, threshold, ratio, mut=()):
    """the scan over an admitted subset of rows: feature_matching.rs:37-81 with `if !admitted[i][j] { continue }` at the top of
    the inner loop.  admitted: bool (n0, n1)."""
    admitted = np.asarray(admitted, bool).reshape(len(d0), len(d1))
    return match_from_distances(distances(d0, d1, mut), threshold, ratio, mut, admitted)
