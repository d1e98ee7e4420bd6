"""Planes and keypoints for the two keypoint ops (k_orientation, k_mldb), shared by the GPU tests (tests/test_gpu_describe.py)
and the host proof that they have teeth (tests/test_describe_teeth_host.py).  Built from seeds and from the arithmetic of the
numpy statement (tests/mldb_numpy.py) alone: neither the oracle nor the product is imported.  TEST INFRASTRUCTURE ONLY.

A level is a dict with the keys w, h, octave and esigma, as the library's plan_levels gives them; every builder takes the
level list.  Four families:

  crafted   made-up planes of four kinds, keypoints at and beyond the border at degenerate scales, angles and octaves
  nonfinite NaN, the infinities and 1e30 as keypoint fields
  tie       keypoints placed so that ONE lattice sample lies within an ulp of a rounding boundary: two associations of
            descriptors.rs:112-113 round it to different pixels
  mirror    planes tiled with blocks that are mirror-symmetric about a keypoint: mirrored cells hold the same samples in
            the opposite order, so their means differ by the rounding of the sums alone, or tie exactly
"""
import numpy as np

import mldb_numpy as M

F = np.float32
KINDS = ("wide", "ints", "flat_gradients", "ly_not_positive")
SPECIAL_ANGLES = [0.0, -0.0, np.pi / 4, -np.pi / 4, 3 * np.pi / 4, -3 * np.pi / 4, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 1000.0]
ANGLES = np.array(SPECIAL_ANGLES + list(np.linspace(-np.pi, np.pi, 14)[1:-1]), np.float32)  # 23 of them
OCTAVES = (0, 0, -1, 1, 0, 30, 0)  # relative to the level's octave; 30: the largest the entry point accepts


def crafted_planes(levels, kind, seed):
    """Lt, Lx, Ly of every level, made up: the ops under test read planes, not images.
    wide: both signs over 40 binades and no two pixels alike, so that a sample taken one pixel off, a wrong cell or a
    wrong weight shows.  (It does NOT show a change in the order or the rounding of the descriptor's additions: that moves
    a cell's mean by ulps, and random means are almost never ulps apart.  The mirror family is for that.)
    ints: small integers, so that cell means tie exactly and a `>=` in place of `>` would flip bits; flat_gradients:
    Lx = Ly = 0, no orientation window is longer than zero and the given angle has to come back; ly_not_positive: every
    orientation sample skipped."""
    rng = np.random.default_rng(seed)
    out = []
    for lv in levels:
        shape = (lv["h"], lv["w"])

        def wide():
            return (rng.choice([-1.0, 1.0], shape) * np.exp2(rng.uniform(-20, 20, shape)) * rng.uniform(1, 2, shape)).astype(np.float32)

        if kind == "wide":
            p = dict(Lt=wide(), Lx=wide(), Ly=wide())
        elif kind == "ints":
            p = {n: rng.integers(-2, 3, shape).astype(np.float32) for n in ("Lt", "Lx", "Ly")}
        elif kind == "flat_gradients":
            p = dict(Lt=wide(), Lx=np.zeros(shape, np.float32), Ly=np.zeros(shape, np.float32))
        else:
            ly = -np.abs(wide())
            ly[rng.uniform(size=shape) < 0.2] = 0.0
            ly[rng.uniform(size=shape) < 0.1] = -0.0
            p = dict(Lt=wide(), Lx=wide(), Ly=ly)
        out.append(p)
    return out


def crafted_keypoints(levels):
    """Per level: 10 x 9 positions (the corners, the edges, a few pixels outside, exactly w - 1, halves) x 6 sizes (scale 0,
    1, 3, the level's natural one, ten planes wide, negative); octave and angle cycle through OCTAVES and ANGLES with the
    running index (7 and 23 are coprime to each other and to the 540 keypoints of a level, so every pairing turns up).
    The position is given in LEVEL pixels of the descriptor, which divides by the keypoint's own octave."""
    rows = []
    i = 0
    for lvl, lv in enumerate(levels):
        lw, lh, o = lv["w"], lv["h"], lv["octave"]
        xs = [-3.0, 0.0, 0.5, 2.5, lw // 2 + 0.5, lw - 1.5, lw - 1.0, lw + 2.0, lw + 5.0, lw + 9.0]
        ys = [-3.0, 0.0, 0.5, 2.5, lh // 4 + 0.25, lh // 2 + 0.5, lh - 1.5, lh - 1.0, lh + 2.0]
        sizes = [0.0, 2.0, 6.0, lv["esigma"] * 1.5 / 2 ** o, 2.0 * lw, -4.0]  # in level pixels: scale = round(size / 2)
        for py in ys:
            for px in xs:
                for sz in sizes:
                    rel = OCTAVES[i % len(OCTAVES)]
                    okp = 30 if rel == 30 else max(0, o + rel)
                    r = 2.0 ** okp
                    rows.append((px * r, py * r, 0.0, sz * r, okp, lvl, ANGLES[i % len(ANGLES)], 0))
                    i += 1
    return np.array(rows, M.KEYPOINT_DTYPE)


def nonfinite_keypoints(levels):
    rows = []
    vals = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    for lvl, lv in enumerate(levels):
        r = 2.0 ** lv["octave"]
        base = [(lv["w"] // 2) * r, (lv["h"] // 3) * r, 0.0, 4.0 * r, lv["octave"], lvl, 0.37, 0]
        for field in (0, 1, 3, 6):  # x, y, size, angle
            for v in vals:
                row = list(base)
                row[field] = v
                rows.append(tuple(row))
        for v in vals:  # ... and all four at once
            rows.append((v, v, 0.0, v, lv["octave"], lvl, v, 0))
        rows.append((np.inf, -np.inf, 0.0, np.nan, 30, lvl, -np.inf, 0))
    return np.array(rows, M.KEYPOINT_DTYPE)


def as_tuples(planes):
    """[{Lt, Lx, Ly}] as the statement takes them: [(Lt, Lx, Ly)]"""
    return [(p["Lt"], p["Lx"], p["Ly"]) for p in planes]


# ---------------------------------------------------------------------------------------------------------------- tie
TIE_SCALES = (3.0, 5.0, 6.0, 7.0)   # not powers of two: a product with the scale rounds
TIE_VARIANTS = ("desc_hoist", "desc_fused")
TIE_META = np.dtype([("coord", "u1"), ("k", "i1"), ("l", "i1"), ("variant", "u1"), ("sign", "i1")])


def lattice_offsets(angle, scale, k, l, mut=()):
    """the offsets (oy, ox) that descriptors.rs:112-113 adds to yf and xf for the lattice point (k, l), from the statement"""
    co, si = M.cosf(angle), M.sinf(angle)
    lf, kf = F(l) + F(0.5), F(k) + F(0.5)
    zero = np.zeros_like(co)
    return M._lattice(zero, lf, co, kf, si, scale, mut), M._lattice(zero, -lf, si, kf, co, scale, mut)


def tie_rounds_apart(kps, meta):
    """per tie keypoint: whether the statement's sample expression and the variant's round the keypoint's own lattice point
    to different pixels in the tie coordinate -- recomputed from the keypoint record alone"""
    out = np.zeros(len(kps), bool)
    ratio = M._ratio(kps["octave"])
    scale = M.round_f32(F(0.5) * kps["size"] / ratio)
    xf, yf = kps["x"] / ratio, kps["y"] / ratio
    for v, name in enumerate(TIE_VARIANTS):
        for c in (0, 1):
            sel = np.nonzero((meta["variant"] == v) & (meta["coord"] == c))[0]
            a, s, k, l = np.ascontiguousarray(kps["angle"][sel]), scale[sel], meta["k"][sel], meta["l"][sel]
            base = (yf, xf)[c][sel]
            o1, o2 = lattice_offsets(a, s, k, l)[c], lattice_offsets(a, s, k, l, (name,))[c]
            out[sel] = M.round_f32(base + o1) != M.round_f32(base + o2)
    return out


def tie_keypoints(levels, planes, seed, per_slot=2):
    """Keypoints one of whose lattice samples is decided by the last bit of descriptors.rs:112-113.  Per level, coordinate
    (0: y, 1: x), sign of (variant - statement), scale of TIE_SCALES and variant of TIE_VARIANTS, `per_slot` keypoints:
    an angle (a special one every third draw) and a lattice point (k, l) are drawn until the statement's offset v1 and the
    variant's v2 differ in f32; then the coordinate is put next to n + 0.5 - v so that round(c + v1) != round(c + v2), the
    other coordinate near the middle of the plane, and the draw is kept if the two pixels lie inside the plane and differ in
    Lt (so that the moved sample moves a mean).  Octave and level are the level's own; the angle is the given one.
    Returns (keypoints, meta): meta says which lattice point, coordinate and variant a keypoint was built for."""
    rng = np.random.default_rng(seed)
    rows, meta = [], []
    special = np.array(SPECIAL_ANGLES[:-1], F)
    for lvl, lv in enumerate(levels):
        lw, lh, r = lv["w"], lv["h"], 2.0 ** lv["octave"]
        lt = planes[lvl]["Lt"]
        for coord in (0, 1):
            for sign in (-1, 1):
                for scale in TIE_SCALES:
                    for v, name in enumerate(TIE_VARIANTS):
                        found = draws = 0
                        while found < per_slot:
                            if draws % 64 == 0:  # 64 draws at a time: an angle (every third a special one) and (k, l)
                                assert draws < 20000, (lvl, coord, sign, scale, name)
                                angs = rng.uniform(-np.pi, np.pi, 64).astype(F)
                                angs[::3] = special[rng.integers(len(special), size=22)]
                                ks, ls = rng.integers(-10, 11, 64), rng.integers(-10, 11, 64)
                                sc = np.full(64, scale, F)
                                b1 = lattice_offsets(angs, sc, ks, ls)
                                b2 = lattice_offsets(angs, sc, ks, ls, (name,))
                            d = draws % 64
                            draws += 1
                            ang, k, l = angs[d:d + 1], int(ks[d]), int(ls[d])
                            o1, o2 = (b1[0][d:d + 1], b1[1][d:d + 1]), (b2[0][d:d + 1], b2[1][d:d + 1])
                            v1, v2 = o1[coord][0], o2[coord][0]
                            if not (v2 > v1 if sign > 0 else v2 < v1):
                                continue
                            dim, odim = (lh, lw) if coord == 0 else (lw, lh)
                            # the keypoint near the middle of the plane, so that as much of the lattice as fits stays inside
                            n = int(np.floor(dim / 2 + float(v1))) + int(rng.integers(-3, 4))
                            other = F(odim // 2 + int(rng.integers(-3, 4)) + rng.choice([0.0, 0.25, 0.5]))
                            c0 = F(F(n + 0.5) - max(v1, v2))
                            c = None
                            for cand in (c0, np.nextafter(c0, F(np.inf)), np.nextafter(c0, F(-np.inf))):
                                if M.round_f32(F(cand + v1)) != M.round_f32(F(cand + v2)):
                                    c = F(cand)
                                    break
                            if c is None:
                                continue
                            pa, pb = int(M.round_f32(F(c + v1))), int(M.round_f32(F(c + v2)))
                            po = int(M.round_f32(F(other + o1[1 - coord][0])))
                            if M.round_f32(F(other + o2[1 - coord][0])) != po:
                                continue  # (the other coordinate has to stay: ONE sample moves by ONE pixel)
                            if min(pa, pb) < 0 or max(pa, pb) > dim - 1 or po < 0 or po > odim - 1:
                                continue
                            va, vb = (lt[pa, po], lt[pb, po]) if coord == 0 else (lt[po, pa], lt[po, pb])
                            if va == vb:
                                continue
                            yf, xf = (c, other) if coord == 0 else (other, c)
                            rows.append((F(xf) * F(r), F(yf) * F(r), 0.0, 2.0 * scale * r, lv["octave"], lvl, ang[0], 0))
                            meta.append((coord, k, l, v, sign))
                            found += 1
    return np.array(rows, M.KEYPOINT_DTYPE), np.array(meta, TIE_META)


# ------------------------------------------------------------------------------------------------------------- mirror
MIRROR_PITCH = 22   # a block, one pixel of margin on each side
MIRROR_ANGLES = (0.0, -0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2)
MIRROR_META = np.dtype([("odd", "u1"), ("bx", "u2"), ("by", "u2")])
# the lattice direction along the image's (x, y) at each angle: x = xf + sx * (k or l) + ..., y = yf + sy * (l or k) + ...
_MIRROR_SIGNS = {0: (1, 1), 1: (1, 1), 2: (-1, -1), 3: (-1, -1), 4: (-1, 1), 5: (1, -1)}


def mirror_block_starts(dim):
    """first pixels of the blocks along an axis of `dim` pixels: every sample of a keypoint at a block's centre, the 3 x 3
    grid's included, lies in [start - 1, start + 20], inside the plane"""
    return list(range(1, dim - 21, MIRROR_PITCH))


def mirror_planes(levels, seed):
    """Lt, Lx, Ly of every level, tiled with blocks (pitch 22 from pixel 1) that are mirror-symmetric in x and in y about
    their own centre; noise of the same kind in between.  Blocks alternate, like a chessboard, between two conventions:
      even  20 x 20 pixels [s, s + 19], symmetric about s + 9.5.  At scale 1 a keypoint at (s + 9.5, s + 9.5) puts the samples
            of the 2 x 2 and 4 x 4 grids (k, l in [-10, 10)) on the block's pixels: mirrored cells hold mirrored samples.
      odd   21 x 21 pixels [s, s + 20], symmetric about pixel s + 10.  The 3 x 3 grid has step 7 and k, l in [-10, 11): at
            angle 0 its samples are xf + 0.5 - 10 .. xf + 0.5 + 10, centred half a pixel above the keypoint, so the keypoint
            sits at s + 9.5 where the lattice runs up the axis and at s + 10.5 where it runs down.
    All magnitudes lie in [1, 2), one binade, with random signs: the rounding of a cell's sum is then large against the
    difference of two mirrored sums, which is zero.  (Positive values alone were tried too: mirrored means are as close, but
    all sums then share a binade and dropping or cheapening the division by nsamples changed no bit at 1 and 3 channels.)"""
    rng = np.random.default_rng(seed)
    out = []
    for lv in levels:
        shape = (lv["h"], lv["w"])

        def draw(shp):
            return (rng.uniform(1, 2, shp) * rng.choice([-1.0, 1.0], shp)).astype(np.float32)

        p = {}
        for name in ("Lt", "Lx", "Ly"):
            a = draw(shape)
            for by, sy in enumerate(mirror_block_starts(lv["h"])):
                for bx, sx in enumerate(mirror_block_starts(lv["w"])):
                    odd = (bx + by) % 2
                    q = draw((11, 11))[:10 + odd, :10 + odd]               # a quarter (the odd block's has the centre lines)
                    half = np.concatenate([q, q[:, ::-1][:, odd:]], axis=1)
                    a[sy:sy + 20 + odd, sx:sx + 20 + odd] = np.concatenate([half, half[::-1][odd:]], axis=0)
            p[name] = a
        out.append(p)
    return out


def mirror_keypoints(levels):
    """One keypoint per block and angle of MIRROR_ANGLES, scale 1, at the block's centre by the block's convention (see
    mirror_planes).  At these angles cos and sin are 0, +-1 or below 1e-7 in magnitude: every sample coordinate is an
    integer plus at most a few ulp, the lattice maps cells onto cells, and a cell's mirror image is a cell.  Returns
    (keypoints, meta)."""
    rows, meta = [], []
    for lvl, lv in enumerate(levels):
        r = 2.0 ** lv["octave"]
        for by, sy in enumerate(mirror_block_starts(lv["h"])):
            for bx, sx in enumerate(mirror_block_starts(lv["w"])):
                odd = (bx + by) % 2
                for a, ang in enumerate(MIRROR_ANGLES):
                    dx, dy = _MIRROR_SIGNS[a]
                    xf = sx + 9.5 + (0.5 - 0.5 * dx if odd else 0.0)
                    yf = sy + 9.5 + (0.5 - 0.5 * dy if odd else 0.0)
                    rows.append((xf * r, yf * r, 0.0, 2.0 * r, lv["octave"], lvl, ang, 0))
                    meta.append((odd, bx, by))
    return np.array(rows, M.KEYPOINT_DTYPE), np.array(meta, MIRROR_META)


def _mirror_pairs(odd):
    """index pairs (a, b) of cells that are mirror images in k or in l, in the grids that mirror under the convention"""
    pairs = []
    for base, ng in (((4, 3),) if odd else ((0, 2), (13, 4))):
        for ci in range(ng):
            for cj in range(ng):
                for mi, mj in ((ng - 1 - ci, cj), (ci, ng - 1 - cj)):
                    a, b = base + ci * ng + cj, base + mi * ng + mj
                    if a < b:
                        pairs.append((a, b))
    return pairs


def mirror_closeness(values, meta, channels, ulps=4):
    """from the statement's cell means [29, 3, n]: (pairs, close, tied) -- the number of (keypoint, channel, mirrored cell
    pair)s, how many of them have means within `ulps` float32 steps of each other, and how many are equal"""
    total = close = tied = 0
    for odd in (0, 1):
        sel = np.nonzero(meta["odd"] == odd)[0]
        for a, b in _mirror_pairs(odd):
            for ch in range(channels):
                va, vb = values[a, ch, sel], values[b, ch, sel]
                total += len(sel)
                close += int((np.abs(va - vb) <= ulps * np.spacing(np.maximum(np.abs(va), np.abs(vb)))).sum())
                tied += int((va == vb).sum())
    return total, close, tied
