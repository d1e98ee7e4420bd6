"""Crafted Ldet pyramids for keypoint detection (find_scale_space_extrema + do_subpixel_refinement), shared by
tests/test_extrema_host.py and tests/test_gpu_crafted_extrema.py.  TEST INFRASTRUCTURE ONLY; needs numpy and
tests/extrema_numpy.py, nothing else.

A case is a function returning (w, h, Config overrides, {level: Ldet}): planes of a constant background (0, below every
threshold) with isolated peaks of chosen float32 values, finite throughout.  Besides the peaks its docstring speaks of, every
case but `dense` carries FILL far-away filler keypoints on level 0 (Planes.fill).  pyramid() completes it: the Config as a namespace,
the levels, an Ldet for every level.  Every position is derived from the border test's admissible box as the statement computes
it (extrema_numpy.admissible_box), and every case asserts the float32 facts it relies on (a size that is exactly 3.0, a
squared size that is exactly 12.5, ...), so a change of the arithmetic makes the case fail loudly, not pass emptily.

The configs.  `size` = esigma * derivative_factor as float32; a level of octave 1 stores x * 2 + 0.5.
  E   2 sublevels x 2 octaves, 1.0 x 2.0:   sizes 2, 2.83, 4, 5.66      (levels 0 and 2 exact)
  O   ... 1.5 / sqrt(2) x 2.0:              sizes 2.12, 3, 4.24, 6      (levels 1 and 3 exact)
  V   ... 1.25 x 2.0:                       sizes 2.5, 3.54, 5, 7.07    (level 2 exact: 25 = 3^2 + 4^2 across the octave change)
  M   4 sublevels x 2 octaves, b x 2.0 with b such that level 3 (the last of octave 0) has size^2 == 12.5 = 2.5^2 + 2.5^2
      and level 4 (the first of octave 1) has size^2 < 18 = 3^2 + 3^2: the one geometry in which the second pass of
      :110-129 drops anything at all.  (An entry B of level L is dropped for a LATER entry C of level L + 1 within size(L) of
      it.  In the first pass C looked at B with the larger size(L + 1); within one octave C's query point is its stored
      point, so B would have been hit and C, first hit or not, would sit at or before B's position or be gone.  Only across
      an octave change do the two points differ, by (0.5, 0.5).)
  G   1 level, 2.5 x 2.0: size 5: a checkerboard of peaks has ~19 earlier neighbours within `size`: more than the device's
      lists (12) and reverse lists (12) hold
  default   Config::default(): 4 x 4 (two octaves at these shapes), size 2.4 on level 0
"""
from types import SimpleNamespace

import numpy as np

import extrema_numpy as E

F = np.float32
DEFAULTS = dict(num_sublevels=4, max_octave_evolution=4, base_scale_offset=1.6, derivative_factor=1.5, detector_threshold=0.001)
CFG_E = dict(num_sublevels=2, max_octave_evolution=2, base_scale_offset=1.0, derivative_factor=2.0)
CFG_O = dict(num_sublevels=2, max_octave_evolution=2, base_scale_offset=1.5 / 2.0 ** 0.5, derivative_factor=2.0)
CFG_V = dict(num_sublevels=2, max_octave_evolution=2, base_scale_offset=1.25, derivative_factor=2.0)
CFG_M = dict(num_sublevels=4, max_octave_evolution=2, base_scale_offset=1.0511205187985486, derivative_factor=2.0)
CFG_G = dict(num_sublevels=1, max_octave_evolution=1, base_scale_offset=2.5, derivative_factor=2.0)
BG = F(0.0)
SHAPES = ((200, 192), (202, 190))  # level widths 200 / 100: k_nms's float4 path; 202 / 101: its scalar path
DENSE_SHAPE = (208, 200)           # its own: the device selection's hand-back makes the context skip the device for the next jobs of that shape
FILL = 20                          # filler keypoints per case (Planes.fill)


def up(v):
    return np.nextafter(F(v), F(np.inf))


def config(overrides):
    return SimpleNamespace(**{**DEFAULTS, **overrides})


def levels_of(w, h, overrides):
    cfg = config(overrides)
    return E.plan_levels(w, h, cfg.num_sublevels, cfg.max_octave_evolution, cfg.base_scale_offset)


class Planes:
    """the Ldet planes of a case under construction"""

    def __init__(self, w, h, overrides):
        self.w, self.h, self.overrides = w, h, overrides
        self.cfg = config(overrides)
        self.levels = levels_of(w, h, overrides)
        self.planes = {}

    def size(self, level):
        return E.level_size(self.levels[level], self.cfg)[0]

    def box(self, level):
        b = E.admissible_box(self.levels[level], self.cfg)
        assert b is not None, (level, "no admissible interior")
        return b

    def centre(self, level):
        x0, x1, y0, y1 = self.box(level)
        return (x0 + x1) // 2, (y0 + y1) // 2

    def put(self, level, x, y, v, inside=True):
        """a pixel value; `inside`: what the border test must say of the pixel (None: not asked)"""
        lw, lh = self.levels[level][0], self.levels[level][1]
        assert 1 <= x < lw - 1 and 1 <= y < lh - 1, (level, x, y)
        d = self.planes.setdefault(level, np.full((lh, lw), BG, F))
        assert d[y, x] == BG, (level, x, y, "occupied")
        if inside is not None:
            assert bool(E.is_out(x, y, self.levels[level], self.cfg)) != inside, (level, x, y, inside)
        d[y, x] = F(v)
        assert np.isfinite(d[y, x])

    def fill(self, n):
        """n isolated peaks of 0.5 on level 0, on a grid of step 8 inside its admissible box, every one at least 16
        full-resolution pixels (more than twice the largest size here) from every pixel the case has set on any level: they
        meet nothing and each is a keypoint.  They bring every case's candidate count above the 16 that the smallest
        candidate list holds, so that the overflow retry of the extrema pass is taken."""
        taken = []
        for l, d in self.planes.items():
            ratio = 2 ** self.levels[l][2]
            ys, xs = np.nonzero(d != BG)
            taken += [(int(x) * ratio, int(y) * ratio) for x, y in zip(xs, ys)]
        x0, x1, y0, y1 = self.box(0)
        spots = [(x, y) for y in range(y0 + 6, y1 - 5, 8) for x in range(x0 + 6, x1 - 5, 8)
                 if all(max(abs(x - tx), abs(y - ty)) >= 16 for tx, ty in taken)]
        assert len(spots) >= n and self.size(0) < F(4.0), (len(spots), n)
        for x, y in spots[:n]:
            self.put(0, x, y, 0.5)

    def done(self, fill=FILL):
        if fill:
            self.fill(fill)
        return self.w, self.h, self.overrides, self.planes


def pyramid(case):
    """(w, h, cfg namespace, levels, [Ldet of every level]) of a case"""
    w, h, overrides, planes = case
    levels = levels_of(w, h, overrides)
    ldets = [np.ascontiguousarray(planes[l], F) if l in planes else np.full((lv[1], lv[0]), BG, F) for l, lv in enumerate(levels)]
    for l, lv in enumerate(levels):
        assert ldets[l].shape == (lv[1], lv[0]) and np.isfinite(ldets[l]).all()
    return w, h, config(overrides), levels, ldets


def aux_planes(levels, seed):
    """seeded random Lt, Lx, Ly for every level (orientation and descriptors read them)"""
    rng = np.random.default_rng(seed)
    return [{n: rng.standard_normal((lv[1], lv[0])).astype(F) for n in ("Lt", "Lx", "Ly")} for lv in levels]


# ---- a. the strict maximum and the threshold ---------------------------------------------------------------------------------
def case_strict(w, h):
    """Per level 0 and 2: a pair tied across the right edge of a k_nms thread's four pixels (x % 4 == 3 with x + 1), one across
    the left edge (x % 4 == 0 with x - 1), a vertical pair; a peak equal to the threshold; one an ulp above it; an ordinary
    one.  Every member of a pair equals one neighbour: none is a candidate.  Two keypoints per level."""
    p = Planes(w, h, CFG_E)
    thr = F(p.cfg.detector_threshold)
    for level in (0, 2):
        x0, _, y0, _ = p.box(level)
        xa = (x0 + 4) // 4 * 4 + 4  # a multiple of 4 inside the box
        r = [y0 + 3 + 8 * k for k in range(4)]
        p.put(level, xa + 3, r[0], 0.5)
        p.put(level, xa + 4, r[0], 0.5)
        p.put(level, xa + 8, r[1], 0.5)
        p.put(level, xa + 7, r[1], 0.5)
        p.put(level, xa, r[2], 0.5)
        p.put(level, xa, r[2] + 1, 0.5)
        p.put(level, xa, r[3], thr)
        p.put(level, xa + 8, r[3], up(thr))
        p.put(level, xa + 16, r[3], 0.25)
    return p.done()


# ---- b. the descriptor border ------------------------------------------------------------------------------------------------
def case_border(w, h):
    """On every level and every side: a peak on the outermost admitted pixel and one on the innermost refused pixel.  Four
    keypoints per level (two of the admitted peaks sit in the box's corners and serve two sides each)."""
    p = Planes(w, h, CFG_E)
    for level in range(len(p.levels)):
        x0, x1, y0, y1 = p.box(level)
        xc = (x0 + x1) // 2 + 1
        p.put(level, x0, y0, 0.5)                       # left and top, admitted
        p.put(level, x1, y1, 0.5)                       # right and bottom, admitted
        p.put(level, xc, y0, 0.5)                       # top, admitted
        p.put(level, xc - 1, y1, 0.5)                   # bottom, admitted
        p.put(level, x0 - 1, y1, 0.5, inside=False)     # left, refused
        p.put(level, x1 + 1, y0, 0.5, inside=False)     # right, refused
        p.put(level, xc - 3, y0 - 1, 0.5, inside=False)  # top, refused
        p.put(level, xc + 2, y1 + 1, 0.5, inside=False)  # bottom, refused
    return p.done()


# ---- c. dist <= size * size --------------------------------------------------------------------------------------------------
def case_dist_same_level(w, h):
    """Level 0 of E (size 2: 4 = 2^2 + 0^2) and level 1 of O (size 3: 9 = 3^2 + 0^2) cannot share a pyramid; this is E.
    Pairs at (2, 0) and (0, 2): merged (the later, smaller one goes); at (2, 1) and (1, 2): 5 > 4, both stay."""
    p = Planes(w, h, CFG_E)
    assert p.size(0) == F(2.0)
    cx, cy = p.centre(0)
    for k, (dx, dy) in enumerate(((2, 0), (0, 2), (2, 1), (1, 2))):
        x, y = cx - 40 + 20 * k, cy
        p.put(0, x, y, 0.5)
        p.put(0, x + dx, y + dy, 0.4)
    return p.done()


def case_dist_same_level_size3(w, h):
    """Level 1 of O: size 3.  (3, 0) and (0, 3) merge; (3, 1) and (1, 3) (10 > 9) do not."""
    p = Planes(w, h, CFG_O)
    assert p.size(1) == F(3.0)
    cx, cy = p.centre(1)
    for k, (dx, dy) in enumerate(((3, 0), (0, 3), (3, 1), (1, 3))):
        x, y = cx - 40 + 20 * k, cy
        p.put(1, x, y, 0.5)
        p.put(1, x + dx, y + dy, 0.4)
    return p.done()


def case_dist_prev_level(w, h):
    """O: a candidate of level 1 (size 3) against an entry of level 0, same octave.  At (3, 0) and (0, -3) it is within `size`
    of the entry and, smaller, goes; at (3, 1) it stays (and the level-0 entry, size^2 = 4.5, is not dropped for it)."""
    p = Planes(w, h, CFG_O)
    assert p.size(1) == F(3.0)
    cx, cy = p.centre(1)
    for k, (dx, dy) in enumerate(((3, 0), (0, -3), (3, 1))):
        x, y = cx - 30 + 20 * k, cy
        p.put(0, x, y, 0.5)
        p.put(1, x + dx, y + dy, 0.4)
    return p.done()


def case_dist_prev_level_octave(w, h):
    """V: a candidate of level 2 (octave 1, size 5) at level pixel c queries (2 cx, 2 cy) against entries of level 1 (octave 0,
    whole-pixel positions).  Entry at query + (3, 4): 25 <= 25, the candidate goes; entry at query + (1, 5): 26, both stay."""
    p = Planes(w, h, CFG_V)
    assert p.size(2) == F(5.0)
    cx, cy = p.centre(2)
    for k, (dx, dy) in enumerate(((3, 4), (1, 5))):
        x, y = cx - 4 + 8 * k, cy
        p.put(2, x, y, 0.4)
        p.put(1, 2 * x + dx, 2 * y + dy, 0.5)
    return p.done()


def case_dist_next_level(w, h):
    """M: the second pass.  Entry B of level 3 at query + (3, 3) of a level-4 candidate C: the first pass does not see it
    (18 > size(4)^2), C is appended later; B's stored distance to C is (2.5, 2.5): 12.5 <= 12.5, B goes.  B' at query' + (4, 2):
    (3.5, 1.5) is 14.5, B' stays."""
    p = Planes(w, h, CFG_M)
    s3, s4 = p.size(3), p.size(4)
    assert F(s3 * s3) == F(12.5) and F(17.0) < F(s4 * s4) < F(18.0), (s3, s4)
    cx, cy = p.centre(4)
    for k, (dx, dy) in enumerate(((3, 3), (4, 2))):
        x, y = cx - 6 + 12 * k, cy
        p.put(4, x, y, 0.4)
        p.put(3, 2 * x + dx, 2 * y + dy, 0.5)
    return p.done()


def case_dist_default(w, h):
    """Config::default(), level 0, size 2.4 (5.76): (1, 2) is inside, (2, 2) outside; and a peak equal to the default threshold."""
    p = Planes(w, h, {})
    assert abs(float(p.size(0)) - 2.4) < 1e-6
    cx, cy = p.centre(0)
    p.put(0, cx - 10, cy, 0.5)
    p.put(0, cx - 9, cy + 2, 0.4)
    p.put(0, cx + 10, cy, 0.5)
    p.put(0, cx + 12, cy + 2, 0.4)
    p.put(0, cx, cy + 20, F(p.cfg.detector_threshold))  # (the default threshold as float32, met exactly: no candidate)
    return p.done()


# ---- d. a strictly larger response replaces, in place ----------------------------------------------------------------------
def case_response(w, h):
    """Levels 0 and 2 of E.  A, then Z far away, then A2 within `size` of A with A's response: A2 goes, A stays.  B, Zb, then
    B2 within `size` of B and one ulp larger: B2 takes B's cache position, so it comes BEFORE Zb in the output."""
    p = Planes(w, h, CFG_E)
    for level in (0, 2):
        cx, cy = p.centre(level)
        x = cx - 10
        p.put(level, x, cy - 6, 0.5)
        p.put(level, x + 12, cy - 6, 0.45)
        p.put(level, x + 1, cy - 5, 0.5)
        p.put(level, x, cy + 4, 0.5)
        p.put(level, x + 12, cy + 4, 0.45)
        p.put(level, x + 1, cy + 5, up(0.5))
    return p.done()


# ---- e. order ------------------------------------------------------------------------------------------------------------------
def case_order_first_hit(w, h):
    """O, level 1 (size 3).  C within `size` of two entries E1 (earlier) and E2: E1 alone decides -- smaller than C: C takes
    its place; larger: C goes, whatever E2 is.  A chain: B replaces A, then C near B's place but not A's is compared with B
    (and goes); C2 near A's OLD place but not B's sees nothing and is appended."""
    p = Planes(w, h, CFG_O)
    assert p.size(1) == F(3.0)
    cx, cy = p.centre(1)
    x, y = cx - 30, cy - 20
    p.put(1, x, y, 0.3); p.put(1, x + 4, y, 0.7); p.put(1, x + 2, y + 2, 0.5)            # E1 < C < E2: C replaces E1
    x = cx + 10
    p.put(1, x, y, 0.7); p.put(1, x + 4, y, 0.3); p.put(1, x + 2, y + 2, 0.5)            # E1 > C > E2: C goes
    x, y = cx - 30, cy + 10
    p.put(1, x, y, 0.3); p.put(1, x + 2, y + 2, 0.5); p.put(1, x + 4, y + 4, 0.4)        # A, B replaces A, C near B only
    x = cx + 10
    p.put(1, x, y, 0.3); p.put(1, x + 3, y, 0.5); p.put(1, x - 1, y + 2, 0.4)            # A, B replaces A, C2 near A's old place
    return p.done()


def case_order_second_pass_earlier(w, h):
    """E.  F and B of level 1, three pixels apart; C of level 2 (larger than F, smaller than B) within `size` of both: F, the
    first, decides and C takes F's position -- BEFORE B.  The second pass of B looks at cache[B..] and does not see C: B stays."""
    p = Planes(w, h, CFG_E)
    cx, cy = p.centre(2)
    p.put(1, 2 * cx - 2, 2 * cy, 0.3)
    p.put(1, 2 * cx + 1, 2 * cy, 0.6)
    p.put(2, cx, cy, 0.5)
    return p.done()


def case_order_second_pass_later(w, h):
    """M, the mirror.  B of level 3 at query + (3, 3) of C (level 4): unseen in the first pass.  F of level 3 at query + (-1, 4),
    later than B in the scan, smaller than C, within size(4) of the query: C takes F's position -- AFTER B -- and B, within
    size(3) of C's stored point, goes in the second pass."""
    p = Planes(w, h, CFG_M)
    s3, s4 = p.size(3), p.size(4)
    assert F(s3 * s3) == F(12.5) and F(17.0) < F(s4 * s4) < F(18.0), (s3, s4)
    cx, cy = p.centre(4)
    p.put(3, 2 * cx + 3, 2 * cy + 3, 0.6)
    p.put(3, 2 * cx - 1, 2 * cy + 4, 0.3)
    p.put(4, cx, cy, 0.5)
    return p.done()


# ---- f. the refinement's gate ----------------------------------------------------------------------------------------------
def case_gate(w, h):
    """Levels 0 and 2 of E.  Peaks of 4 with neighbours of 3 and 1: |d| is exactly 1.0, the keypoint moves a whole level pixel,
    either way, on either axis and on both; with 3 + ulp the offset is 1 + ulp and the survivor is refused."""
    p = Planes(w, h, CFG_E)
    hi = up(3.0)
    assert F(0.5) * (hi - F(1.0)) == up(1.0)
    # (xp, xm, yp, ym)
    nbs = [(3, 1, 0, 0), (1, 3, 0, 0), (0, 0, 3, 1), (0, 0, 1, 3), (3, 1, 1, 3),
           (hi, 1, 0, 0), (1, hi, 0, 0), (0, 0, hi, 1), (0, 0, 1, hi), (3, 1, 1, hi)]
    for level in (0, 2):
        cx, cy = p.centre(level)
        for k, (xp, xm, yp, ym) in enumerate(nbs):
            x, y = cx - 16 + 8 * (k % 5), cy - 4 + 8 * (k // 5)
            p.put(level, x, y, 4.0)
            for dx, dy, v in ((1, 0, xp), (-1, 0, xm), (0, 1, yp), (0, -1, ym)):
                if v:
                    p.put(level, x + dx, y + dy, v, inside=None)
    return p.done()


# ---- g. dense ------------------------------------------------------------------------------------------------------------------
def case_dense(w, h):
    """G: a checkerboard of 720 peaks of distinct values on one level of size 5."""
    p = Planes(w, h, CFG_G)
    assert p.size(0) == F(5.0)
    x0, x1, y0, y1 = p.box(0)
    pts = [(x, y) for y in range(y0 + 4, y0 + 40) for x in range(x0 + 4, x0 + 44) if (x + y) % 2 == 0]
    assert x0 + 44 <= x1 and y0 + 40 <= y1
    vals = np.random.default_rng(7).permutation(len(pts))
    for (x, y), k in zip(pts, vals):
        p.put(0, x, y, F(1.0) + F(k) * F(2.0 ** -12))
    return p.done(fill=0)


def _both(fn):
    return [(f"{fn.__name__[5:]}_{w}x{h}", lambda fn=fn, w=w, h=h: fn(w, h)) for w, h in SHAPES]


def _one(fn, k):
    w, h = SHAPES[k] if isinstance(k, int) else k
    return [(f"{fn.__name__[5:]}_{w}x{h}", lambda: fn(w, h))]


CASES = (_both(case_strict) + _both(case_border) + _one(case_dist_same_level, 0) + _one(case_dist_same_level_size3, 1) +
         _one(case_dist_prev_level, 0) + _one(case_dist_prev_level_octave, 1) + _one(case_dist_next_level, 0) +
         _one(case_dist_default, 1) + _both(case_response) + _one(case_order_first_hit, 1) +
         _one(case_order_second_pass_earlier, 0) + _one(case_order_second_pass_later, 1) + _both(case_gate) + _one(case_dense, DENSE_SHAPE))
CASE_NAMES = [n for n, _ in CASES]
CASE_FN = dict(CASES)
