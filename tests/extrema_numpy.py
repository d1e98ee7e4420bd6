"""A plain numpy / Python statement of keypoint detection -- find_scale_space_extrema and do_subpixel_refinement
(akaze/src/ops/scale_space_extrema.rs:12-189, without the orientation, which tests/mldb_numpy.py states) -- written from the
reference's text, independently of the oracle (oracle/akaze_ref.cpp) and of the product's kernels and host code.  It imports
neither.  TEST INFRASTRUCTURE ONLY.

float32 throughout, every expression in the reference's order (numpy rounds each float32 operation on its own: no fused
multiply-add).  The cache walk of :57-76 is vectorised ACROSS the cache -- every distance is still the reference's expression
on the reference's operands, and "the first entry that qualifies" is the lowest index of the mask.

A level is (w, h, octave, esigma) as akz_plan_level_info gives them (plan_levels() below restates evolution.rs:135-161 so that
the crafted pyramids need no library); cfg is anything with the attributes derivative_factor and detector_threshold.

MUTATIONS.  Every function takes `mut`, a collection of switch names; each switch flips ONE comparison or rule of the
statement.  They exist only so that tests/test_extrema_host.py can prove that the crafted pyramids (tests/extrema_cases.py)
tell the right statement from a wrong one; nothing else may pass a switch.

  nms_ge                    `>=` against the four neighbours (:38-41)
  thr_ge                    `>=` against the threshold (:37)
  dist_lt                   `dist < size * size` in both passes (:66, :120)
  resp_ge                   a response that is EQUAL replaces too (:67)
  gate_lt                   `|b| < 1.0` in the refinement (:170)
  any_hit_not_first         the `break` of :73 is missing: every entry within `size` has its say, the last one last
  second_pass_any_position  the second pass looks at the whole cache, not at cache[i..] (:115)
  prev_level_at_level0      the guard `class_id != 0` of :59 taken one level too high (`class_id > 1`): a candidate of
                            level 1 does not look at level 0, the one previous level that IS level 0.  (Dropping the guard
                            itself changes no result: while level 0 is scanned the cache holds level 0 only.)
  border_lo_le, border_hi_gt   `left_x <= 0`, `up_y <= 0` / `right_x > w`, `down_y > h` in the border test (:84-87)
"""
import numpy as np

F = np.float32
KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("size", "<f4"),
     ("octave", "<u8"), ("class_id", "<u8"), ("angle", "<f4"), ("_pad", "<u4")])
SWITCHES = ("nms_ge", "thr_ge", "dist_lt", "resp_ge", "gate_lt", "any_hit_not_first", "second_pass_any_position",
            "prev_level_at_level0", "border_lo_le", "border_hi_gt")
SMAX = F(10.0) * np.sqrt(F(2.0))  # :14


def _check(mut):
    bad = set(mut) - set(SWITCHES)
    assert not bad, bad
    return frozenset(mut)


def round_f32(x):
    """f32::round: to the nearest integer, halves away from zero"""
    x = np.asarray(x, F)
    t = np.trunc(x)
    return np.where(np.abs(x - t) >= F(0.5), t + np.copysign(F(1), x), t).astype(F)


def plan_levels(w, h, num_sublevels=4, max_octave_evolution=4, base_scale_offset=1.6):
    """allocate_evolutions (types/evolution.rs:135-161) with the plane sizes of the chained half_size (lib.rs:80-90):
    [(w, h, octave, esigma)]"""
    out = []
    lw, lh = int(w), int(h)
    for i in range(max_octave_evolution):
        rfactor = 1.0 / 2.0 ** float(i)
        if not ((int(w * rfactor) >= 80 and int(h * rfactor) >= 40) or i == 0):
            break
        if i > 0:
            lw, lh = lw // 2, lh // 2
        for j in range(num_sublevels):
            out.append((lw, lh, i, base_scale_offset * 2.0 ** (float(j) / float(num_sublevels) + float(i))))
    return out


def level_size(level, cfg):
    """(size, ratio, sigma_size) of a level's keypoints, float32 (:45, :51-52)"""
    _, _, octave, esigma = level
    size = F(float(esigma) * float(cfg.derivative_factor))
    ratio = F(2.0) ** F(octave)
    return size, F(ratio), F(round_f32(size / F(ratio)))


def is_out(x, y, level, cfg, mut=()):
    """the descriptor-border test of :80-87 for the level pixel (x, y) (arrays allowed)"""
    mut = _check(mut)
    w, h = level[0], level[1]
    m = SMAX * level_size(level, cfg)[2]
    fx, fy = np.asarray(x).astype(F), np.asarray(y).astype(F)
    left_x, right_x = round_f32(fx - m) - F(1), round_f32(fx + m) + F(1)
    up_y, down_y = round_f32(fy - m) - F(1), round_f32(fy + m) + F(1)
    lo = (left_x <= F(0), up_y <= F(0)) if "border_lo_le" in mut else (left_x < F(0), up_y < F(0))
    hi = (right_x > F(w), down_y > F(h)) if "border_hi_gt" in mut else (right_x >= F(w), down_y >= F(h))
    return lo[0] | hi[0] | lo[1] | hi[1]


def admissible_box(level, cfg):
    """(x0, x1, y0, y1), inclusive: the level pixels the border test admits, or None if there are none"""
    w, h = level[0], level[1]
    xs = np.arange(w)
    okx = np.nonzero(~is_out(xs, np.full(w, h // 2), level, cfg))[0]
    ys = np.arange(h)
    oky = np.nonzero(~is_out(np.full(h, w // 2), ys, level, cfg))[0]
    if len(okx) == 0 or len(oky) == 0:
        return None
    assert np.array_equal(okx, np.arange(okx[0], okx[-1] + 1)) and np.array_equal(oky, np.arange(oky[0], oky[-1] + 1))
    return int(okx[0]), int(okx[-1]), int(oky[0]), int(oky[-1])


def candidates(ldet, thr_f32, mut=()):
    """:32-42 -- the flat loop (w + 1) .. len - w - 2 with x != 0 (`x != w` never bites: the last column is scanned, its
    "right" neighbour is the next row's first pixel), strictly above the threshold and the four neighbours.
    Returns the flat indices in scan order."""
    mut = _check(mut)
    d = np.ascontiguousarray(ldet, F)
    h, w = d.shape
    flat = d.ravel()
    i = np.arange(w + 1, flat.size - w - 1)
    i = i[i % w != 0]
    v = flat[i]
    thr = F(thr_f32)
    above = (v >= thr) if "thr_ge" in mut else (v > thr)
    nb = [flat[i + 1], flat[i - 1], flat[i - w], flat[i + w]]
    if "nms_ge" in mut:
        peak = (v >= nb[0]) & (v >= nb[1]) & (v >= nb[2]) & (v >= nb[3])
    else:
        peak = (v > nb[0]) & (v > nb[1]) & (v > nb[2]) & (v > nb[3])
    return i[above & peak]


class _Cache:
    """the keypoint cache of :13 as parallel arrays"""

    def __init__(self, cap):
        self.n = 0
        self.x, self.y, self.response, self.size = (np.zeros(cap, F) for _ in range(4))
        self.octave, self.class_id = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        self.lx, self.ly = np.zeros(cap, np.int64), np.zeros(cap, np.int64)

    def put(self, k, x, y, response, size, octave, class_id, lx, ly):
        self.x[k], self.y[k], self.response[k], self.size[k] = x, y, response, size
        self.octave[k], self.class_id[k], self.lx[k], self.ly[k] = octave, class_id, lx, ly


def select(cands_per_level, ldets, levels, cfg, mut=()):
    """:43-129 on the candidates of candidates() (flat indices per level, scan order).  Returns (survivors as a keypoint
    array with the positions of :89-92, their count = the extrema count)."""
    mut = _check(mut)
    cache = _Cache(sum(len(c) for c in cands_per_level) + 1)
    for e_id, idxs in enumerate(cands_per_level):
        w = levels[e_id][0]
        octave = levels[e_id][2]
        size, ratio, _ = level_size(levels[e_id], cfg)
        flat = np.ascontiguousarray(ldets[e_id], F).ravel()
        for i in idxs:
            x, y = int(i) % w, int(i) // w
            response = np.abs(flat[i])
            px, py = F(x) * ratio, F(y) * ratio
            n = cache.n
            cid = cache.class_id[:n]
            if "prev_level_at_level0" in mut:
                lvl_ok = (cid == e_id) | ((e_id > 1) & (cid == e_id - 1))
            else:
                lvl_ok = (cid == e_id) | ((e_id != 0) & (cid == e_id - 1))
            dx, dy = px - cache.x[:n], py - cache.y[:n]
            dist = dx * dx + dy * dy
            near = (dist < size * size) if "dist_lt" in mut else (dist <= size * size)
            hits = np.nonzero(lvl_ok & near)[0]
            id_repeated, is_repeated, is_extremum = 0, False, True
            for k in hits:
                larger = response >= cache.response[k] if "resp_ge" in mut else response > cache.response[k]
                if larger:
                    id_repeated, is_repeated = int(k), True
                else:
                    is_extremum = False
                if "any_hit_not_first" not in mut:
                    break
            if is_extremum and not is_out(x, y, levels[e_id], cfg, mut):
                k = id_repeated if is_repeated else cache.n
                half = F(0.5) * (ratio - F(1.0))
                cache.put(k, F(x) * ratio + half, F(y) * ratio + half, response, size, octave, e_id, x, y)
                if not is_repeated:
                    cache.n += 1
    keep = []
    n = cache.n
    for i in range(n):
        j0 = 0 if "second_pass_any_position" in mut else i
        nxt = cache.class_id[j0:n] == cache.class_id[i] + 1
        dx, dy = cache.x[i] - cache.x[j0:n], cache.y[i] - cache.y[j0:n]
        dist = dx * dx + dy * dy
        s2 = cache.size[i] * cache.size[i]
        near = (dist < s2) if "dist_lt" in mut else (dist <= s2)
        if not (nxt & near).any():
            keep.append(i)
    out = np.zeros(len(keep), KEYPOINT_DTYPE)
    for f in ("x", "y", "response", "size", "octave", "class_id"):
        out[f] = getattr(cache, f)[keep]
    return out, len(keep)


def refine(kps, ldets, mut=()):
    """:141-178 as the reference behaves: the LU solution is discarded, b = (-d_x, -d_y)"""
    mut = _check(mut)
    out = []
    for kp in kps:
        ratio = F(2.0) ** F(kp["octave"])
        x, y = int(round_f32(kp["x"] / ratio)), int(round_f32(kp["y"] / ratio))
        d = ldets[int(kp["class_id"])]
        x_p, x_m, y_p, y_m = F(d[y, x + 1]), F(d[y, x - 1]), F(d[y + 1, x]), F(d[y - 1, x])
        d_x, d_y = F(0.5) * (x_p - x_m), F(0.5) * (y_p - y_m)
        b0, b1 = -d_x, -d_y
        ok = (np.abs(b0) < F(1.0) and np.abs(b1) < F(1.0)) if "gate_lt" in mut else (np.abs(b0) <= F(1.0) and np.abs(b1) <= F(1.0))
        if ok:
            k = kp.copy()
            half = F(0.5) * (ratio - F(1.0))
            k["x"] = (F(x) + b0) * ratio + half
            k["y"] = (F(y) + b1) * ratio + half
            out.append(k)
    return np.array(out, KEYPOINT_DTYPE) if out else np.zeros(0, KEYPOINT_DTYPE)


def detect(ldets, levels, cfg, mut=()):
    """detect_keypoints (:199-203) without the orientation: (keypoints with angle 0, extrema count)"""
    thr = F(float(cfg.detector_threshold))  # `options.detector_threshold as f32`
    cands = [candidates(ldets[l], thr, mut) for l in range(len(levels))]
    ext, n_ext = select(cands, ldets, levels, cfg, mut)
    return refine(ext, ldets, mut), n_ext
