"""The keypoint budget of include/akaze_hip.h (AKZ_BUDGET_*) stated in numpy float32: broadcast dx, dy, d2, a lexsort for the order,
the kept indices sorted.  numpy rounds every float32 operation on its own and never fuses, which is what the header asks for.
Shared by tests/test_keypoint_budget_host.py and tests/test_gpu_keypoint_budget.py (helpers only, no tests)."""
import numpy as np

F32 = np.float32
STRONGEST, SPREAD = 0, 1


def radius2_numpy(x, y, r, robust, rows=512):
    """radius2_i = min over j with r_i < fl(robust * r_j) of fl(fl(dx*dx) + fl(dy*dy)), +inf where no j dominates i"""
    x, y, r = (np.ascontiguousarray(v, F32) for v in (x, y, r))
    rr = F32(robust) * r
    out = np.full(len(x), np.inf, F32)
    for a in range(0, len(x), rows):
        b = min(a + rows, len(x))
        dx = x[a:b, None] - x[None, :]
        dy = y[a:b, None] - y[None, :]
        d2 = dx * dx + dy * dy
        assert d2.dtype == F32
        dom = r[a:b, None] < rr[None, :]
        out[a:b] = np.where(dom, d2, F32(np.inf)).min(axis=1, initial=F32(np.inf))
    return out


def budget_numpy(kp, max_keypoints, mode, robust=0.9):
    """-> (indices uint64 ascending, radius2 float32 [n] or None)"""
    x, y, r = (np.ascontiguousarray(kp[f], F32) for f in ("x", "y", "response"))
    n = len(x)
    if mode == SPREAD:
        rad = radius2_numpy(x, y, r, robust)
        order = np.lexsort((np.arange(n), -r, -rad))  # the last key is the first criterion
    else:
        rad = None
        order = np.lexsort((np.arange(n), -r))
    keep = min(int(max_keypoints), n)
    return np.sort(order[:keep]).astype(np.uint64), rad


def keypoints(amd, x, y, r):
    k = np.zeros(len(x), amd.KEYPOINT_DTYPE)
    k["x"], k["y"], k["response"] = x, y, r
    k["size"] = 4.0
    return k


def lattice(amd, n, seed, side=None, values=(0.25, 0.5, 0.75, 1.0)):
    """n keypoints on an integer lattice (shuffled, row-major cells of a side x side grid, so no two coincide) with responses
    from a set of 4 values: d2, radius and response all tie in many places and only the index decides"""
    rng = np.random.default_rng(seed)
    side = side or int(np.ceil(np.sqrt(n)))
    cells = rng.permutation(side * side)[:n]
    return keypoints(amd, (cells % side).astype(F32), (cells // side).astype(F32), rng.choice(np.asarray(values, F32), n))


def random_set(amd, n, seed, w=1920.0, h=1080.0):
    rng = np.random.default_rng(seed)
    return keypoints(amd, rng.uniform(0, w, n).astype(F32), rng.uniform(0, h, n).astype(F32),
                     (rng.gamma(1.5, 0.004, n) + 0.001).astype(F32))
