"""A plain numpy statement of the two keypoint ops -- compute_main_orientation (akaze/src/ops/scale_space_extrema.rs:205-329)
and get_mldb_descriptor (akaze/src/ops/descriptors.rs:37-175) -- written from the reference's text, independently of the
oracle (oracle/akaze_ref.cpp) and of the product's kernels.  TEST INFRASTRUCTURE ONLY.

float32 throughout and every add in the reference's order: the work is vectorised ACROSS keypoints and sequential over
samples, so each keypoint's chain of additions is the reference's chain.  atan2f / cosf / sinf are the process's libm
(tests/libm_check/liblibm_check.so), not numpy's: np.arctan2 on float32 differs from glibc in the last bit.

Sampling has two forms:

  "reference"  the reference's own indexing, GrayFloatImage::get = buffer[width * y + x] (types/image.rs:95-97), with its
               casts: the orientation's `as usize` (negatives and NaN to 0), the descriptor's `as isize as usize`.  A
               sample with x >= width on a row that is not the last reads the next row.  `completes[i]` says whether every
               index of keypoint i stayed inside [0, w*h) and every descriptor coordinate was non-negative, that is whether
               the reference returns at all (otherwise it panics, or wraps, by build profile; what this module returns for
               such a keypoint is then meaningless, it only stays inside the planes).
  "clamped"    the product's contract: float to int32 saturating with NaN to 0 (the orientation's negatives to 0 first,
               as the reference), then x clamped to [0, w-1] and y to [0, h-1].

MUTATIONS.  main_orientation, mldb_values, mldb_bits, describe_level and describe take `mut`, a collection of switch names;
each switch changes ONE comparison, rule, order or association of the statement.  They exist only so that
tests/test_describe_teeth_host.py can prove that the describe cases (tests/describe_cases.py) tell the right statement from
a nearly right one; nothing else may pass a switch.  Lines are those of scale_space_extrema.rs (ori_*) and descriptors.rs
(desc_*).

  ori_disc_le            `i * i + j * j <= 36`: 113 samples (:288)
  ori_angs_yx            the sample angles as atan2f(res_y, res_x), what :294 presumably meant
  ori_sums_reset         sum_x, sum_y set to zero at the start of every window (:301-302 are outside the loop)
  ori_best_ge            `val >= max` (:323)
  ori_no_wrap            the branch for a window that wraps (ang2 < ang1) missing (:314)
  ori_last_window_off    the loop ends one window early (:304)
  ori_j_outer            the samples visited j outer, i inner (:286-287)
  ori_lx_ly_swapped      res_x from Ly, res_y from Lx (:292-293)
  ori_scale_trunc        s truncated, not rounded (:280)
  ori_weight_off_x       res_x without the Gaussian weight (:292)
  ori_final_xy           the angle as atan2f(sum_x, sum_y) (:326)
  ori_keypoint_octave    the ratio from keypoint.octave, not from the level's (:279)
  ori_edges_f64          ang1, ang2 and 2 pi formed and compared in f64 (:300-310); INVISIBLE, see below
  ori_edges_le           `<=` against ang1, ang2 and 2 pi (:313-314; `ang > 0` stays); INVISIBLE, see below
  round_half_even        f32::round as round-half-to-even, in both ops (:280, :289-290; descriptors.rs:52, :114-115)
  desc_ge                `ival >= values[..]` (:165)
  desc_no_half           the lattice without its 0.5 offsets (:110-111)
  desc_left_assoc        `yf + l * co * scale + k * si * scale`: the parentheses of :112-113 dropped
  desc_hoist             `l * (co * scale) + k * (si * scale)`: co * scale and si * scale formed first (:112-113)
  desc_fused             the first product by scale fused with the addition: l * co taken in f32, then
                         (l * co) * scale + k * si * scale formed in f64 and rounded once (:112-113)
  desc_kl_swapped        a cell's samples added l outer, k inner (:108-109)
  desc_cells_j_outer     the cells visited j outer, i inner (:102-103)
  desc_step_floor        sample_size as floor(pattern_size * multiplier): the 3 x 3 grid's step 6 (:61)
  desc_scale_trunc       scale truncated, not rounded (:52)
  desc_dxdy_swapped      dx takes rry, dy takes rrx (:128-129)
  desc_rot_sign          si negated: the lattice and the gradients turned the other way (:56)
  desc_channel_minor     the comparisons ordered cell pair first, channel last (:161-164)
  desc_msb_first         bits packed from the top of each byte (:170)
  desc_no_div            the sums compared, not the means (:136-138)
  desc_recip             `* (1 / nsamples)` for `/ nsamples` (:136-138)
  desc_sqrt_f64          the 2-channel magnitude as hypot in f64, rounded to f32 once (:124)
  desc_level_octave      the ratio from the level's octave, not from keypoint.octave (:51)

The two invisible switches.  :294 takes atan2f(res_y, res_y), which yields only pi/4, -3 pi/4, +0, -pi and NaN; of these
only pi/4 is above zero, so only it can fall into a window.  No ang1, ang2 or 2 pi, accumulated in f32 or in f64, equals
pi/4 in f32, and both accumulations place pi/4 in the same windows (tests/test_describe_teeth_host.py asserts both).  So
ori_edges_f64 and ori_edges_le change no result on any input (with the sample angles of ori_angs_yx they could, for an angle
that equals an edge or lies between its two accumulations): a change of the window edges in the product cannot be caught
through these ops as long as :294 stands, and must not be "fixed" on one side only.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("size", "<f4"),
     ("octave", "<u8"), ("class_id", "<u8"), ("angle", "<f4"), ("_pad", "<u4")])
F = np.float32
PI = F(np.pi)  # std::f32::consts::PI
SWITCHES = ("ori_disc_le", "ori_angs_yx", "ori_sums_reset", "ori_best_ge", "ori_no_wrap", "ori_last_window_off", "ori_j_outer",
            "ori_lx_ly_swapped", "ori_scale_trunc", "ori_weight_off_x", "ori_final_xy", "ori_keypoint_octave", "ori_edges_f64",
            "ori_edges_le", "round_half_even", "desc_ge", "desc_no_half", "desc_left_assoc", "desc_hoist", "desc_fused",
            "desc_kl_swapped", "desc_cells_j_outer", "desc_step_floor", "desc_scale_trunc", "desc_dxdy_swapped", "desc_rot_sign",
            "desc_channel_minor", "desc_msb_first", "desc_no_div", "desc_recip", "desc_sqrt_f64", "desc_level_octave")
INVISIBLE = ("ori_edges_f64", "ori_edges_le")


def _check(mut):
    bad = set(mut) - set(SWITCHES)
    assert not bad, bad
    return frozenset(mut)

# scale_space_extrema.rs:207-271
GAUSS25 = np.array([
    [0.02546481, 0.02350698, 0.01849125, 0.01239505, 0.00708017, 0.00344629, 0.00142946],
    [0.02350698, 0.02169968, 0.01706957, 0.01144208, 0.00653582, 0.00318132, 0.00131956],
    [0.01849125, 0.01706957, 0.01342740, 0.00900066, 0.00514126, 0.00250252, 0.00103800],
    [0.01239505, 0.01144208, 0.00900066, 0.00603332, 0.00344629, 0.00167749, 0.00069579],
    [0.00708017, 0.00653582, 0.00514126, 0.00344629, 0.00196855, 0.00095820, 0.00039744],
    [0.00344629, 0.00318132, 0.00250252, 0.00167749, 0.00095820, 0.00046640, 0.00019346],
    [0.00142946, 0.00131956, 0.00103800, 0.00069579, 0.00039744, 0.00019346, 0.00008024]], np.float32)

_libm = None


def libm():
    global _libm
    if _libm is None:
        d = os.path.join(HERE, "libm_check")
        subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL)
        _libm = C.CDLL(os.path.join(d, "liblibm_check.so"))
    return _libm


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def atan2f(y, x):
    y, x = np.ascontiguousarray(y, F), np.ascontiguousarray(x, F)
    out = np.empty_like(y)
    libm().lc_atan2f(0, _p(y), _p(x), _p(out), C.c_uint64(y.size))
    return out


def _unary(name, x):
    x = np.ascontiguousarray(x, F)
    out = np.empty_like(x)
    getattr(libm(), name)(0, _p(x), _p(out), C.c_uint64(x.size), None)
    return out


def cosf(x):
    return _unary("lc_cosf", x)


def sinf(x):
    return _unary("lc_sinf", x)


def round_f32(x, mut=()):
    """f32::round: to the nearest integer, halves away from zero; NaN and the infinities pass through."""
    x = np.asarray(x, F)
    if "round_half_even" in mut:
        return np.rint(x).astype(F)
    t = np.trunc(x)
    with np.errstate(invalid="ignore"):
        away = np.abs(x - t) >= F(0.5)  # (x - t is exact; inf - inf = NaN compares false)
    return np.where(away, t + np.copysign(F(1), x), t).astype(F)


_BIG = F(2.0 ** 40)  # beyond every plane, far below what an int64 product with a plane's width can overflow


def _as_usize(v):
    """f32 `as usize`: saturating, NaN and negatives to 0 (values beyond 2^40 stand for "far outside")."""
    v = np.where(np.isnan(v), F(0), v)
    return np.clip(v, F(0), _BIG).astype(np.int64)


def _as_isize(v):
    """f32 `as isize`: saturating, NaN to 0."""
    v = np.where(np.isnan(v), F(0), v)
    return np.clip(v, -_BIG, _BIG).astype(np.int64)


def _as_i32(v):
    """float to int32, saturating, NaN to 0: the product's conversion."""
    v = np.where(np.isnan(v), F(0), v)
    return np.clip(v.astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


class Coverage:
    """What the samples of each keypoint did at the border (filled from the statement's side, no product code)."""

    def __init__(self, n):
        self.left, self.right, self.top, self.bottom = (np.zeros(n, bool) for _ in range(4))  # clamped form: a sample clamped there
        self.next_row = np.zeros(n, bool)   # reference form: a sample with x >= w that stayed inside the buffer
        self.completes = np.ones(n, bool)   # reference form: the reference returns


class _Sampler:
    def __init__(self, w, h, sampling, cov):
        assert sampling in ("reference", "clamped")
        self.w, self.h, self.sampling, self.cov = int(w), int(h), sampling, cov

    def index(self, fx, fy, orientation):
        """flat index of the sample at the rounded float coordinates (fx, fy), per keypoint"""
        w, h, cov = self.w, self.h, self.cov
        if self.sampling == "reference":
            if orientation:
                ix, iy = _as_usize(fx), _as_usize(fy)
                neg = np.zeros(len(ix), bool)
            else:
                ix, iy = _as_isize(fx), _as_isize(fy)
                neg = (ix < 0) | (iy < 0)
            idx = w * iy + ix
            ok = ~neg & (idx >= 0) & (idx < w * h)
            cov.completes &= ok
            cov.next_row |= ok & (ix >= w)
            return np.where(ok, idx, 0)
        if orientation:  # `fx > 0 ? (int)fx : 0`
            with np.errstate(invalid="ignore"):
                fx, fy = np.where(fx > F(0), fx, F(0)), np.where(fy > F(0), fy, F(0))
        ix, iy = _as_i32(fx), _as_i32(fy)
        cov.left |= ix < 0
        cov.right |= ix > w - 1
        cov.top |= iy < 0
        cov.bottom |= iy > h - 1
        return w * np.clip(iy, 0, h - 1) + np.clip(ix, 0, w - 1)


def _ratio(octave):
    return (np.uint64(1) << np.asarray(octave, np.uint64)).astype(F)


def orientation_windows(T=F):
    """the (ang1, ang2) of every window of scale_space_extrema.rs:300-310, ang1 already advanced (it is, before the test);
    T: the type they are formed in (np.float64 from the same f32 constants: the switch ori_edges_f64)"""
    out = []
    pi = T(PI)
    ang1 = T(0)
    while ang1 < T(2.0) * pi:
        ang2 = ang1 - T(5.0) * pi / T(3.0) if ang1 + pi / T(3.0) > T(2.0) * pi else ang1 + pi / T(3.0)
        ang1 = T(ang1 + T(F(0.15)))
        out.append((ang1, T(ang2)))
    return out


def main_orientation(lx, ly, level_octave, kps, sampling, cov=None, mut=()):
    """compute_main_orientation for keypoints of ONE level (its Lx, Ly as 2-D float32 arrays, its octave): the angle of
    every keypoint, the given one where no window's vector is longer than zero."""
    mut = _check(mut)
    n = len(kps)
    h, w = lx.shape
    cov = cov or Coverage(n)
    smp = _Sampler(w, h, sampling, cov)
    lxf, lyf = np.ascontiguousarray(lx, F).ravel(), np.ascontiguousarray(ly, F).ravel()
    if "ori_lx_ly_swapped" in mut:
        lxf, lyf = lyf, lxf
    with np.errstate(all="ignore"):
        ratio = _ratio(np.full(n, level_octave))  # the LEVEL's octave (:279), not the keypoint's
        if "ori_keypoint_octave" in mut:
            ratio = _ratio(kps["octave"])
        s = F(0.5) * kps["size"].astype(F) / ratio
        s = np.trunc(s) if "ori_scale_trunc" in mut else round_f32(s, mut)
        xf, yf = kps["x"].astype(F) / ratio, kps["y"].astype(F) / ratio
        ident = [6, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6]
        res_x, res_y = [], []
        order = [(i, j) for i in range(-6, 7) for j in range(-6, 7)]
        if "ori_j_outer" in mut:
            order = [(i, j) for j in range(-6, 7) for i in range(-6, 7)]
        for i, j in order:
            if (i * i + j * j <= 36) if "ori_disc_le" in mut else (i * i + j * j < 36):
                fy = round_f32(yf + F(j) * s, mut)
                fx = round_f32(xf + F(i) * s, mut)
                p = smp.index(fx, fy, True)
                g = GAUSS25[ident[i + 6]][ident[j + 6]]
                res_x.append(lxf[p] if "ori_weight_off_x" in mut else g * lxf[p])
                res_y.append(g * lyf[p])
        ns = len(res_x)
        assert ns == (113 if "ori_disc_le" in mut else 109)
        res_x, res_y = np.array(res_x, F), np.array(res_y, F)  # [109, n]
        angs = atan2f(res_y, res_x if "ori_angs_yx" in mut else res_y)  # (:294: res_y twice)
        sum_x, sum_y, best = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
        bx, by, found = np.zeros(n, F), np.zeros(n, F), np.zeros(n, bool)
        T = np.float64 if "ori_edges_f64" in mut else F
        le = "ori_edges_le" in mut
        two_pi = T(2.0) * T(PI)
        windows = orientation_windows(T)
        if "ori_last_window_off" in mut:
            windows = windows[:-1]
        for ang1, ang2 in windows:
            if "ori_sums_reset" in mut:
                sum_x, sum_y = np.zeros(n, F), np.zeros(n, F)
            for k in range(ns):
                ang = angs[k].astype(T)
                if ang1 < ang2:
                    take = ((ang1 <= ang) & (ang <= ang2)) if le else ((ang1 < ang) & (ang < ang2))
                elif ang2 < ang1 and "ori_no_wrap" not in mut:
                    if le:
                        take = ((ang > T(0)) & (ang <= ang2)) | ((ang >= ang1) & (ang <= two_pi))
                    else:
                        take = ((ang > T(0)) & (ang < ang2)) | ((ang > ang1) & (ang < two_pi))
                else:
                    take = np.zeros(n, bool)
                sum_x = np.where(take, sum_x + res_x[k], sum_x)
                sum_y = np.where(take, sum_y + res_y[k], sum_y)
            val = sum_x * sum_x + sum_y * sum_y
            new = (val >= best) if "ori_best_ge" in mut else (val > best)
            best = np.where(new, val, best)
            bx, by = np.where(new, sum_x, bx), np.where(new, sum_y, by)
            found |= new
        final = atan2f(bx, by) if "ori_final_xy" in mut else atan2f(by, bx)
        return np.where(found, final, kps["angle"].astype(F)).astype(F)


def _lattice(base, a, ca, b, cb, scale, mut):
    """base + (a * ca * scale + b * cb * scale), descriptors.rs:112-113, float32 and in that order"""
    if "desc_hoist" in mut:
        t = a * (ca * scale) + b * (cb * scale)
    elif "desc_fused" in mut:
        t = ((a * ca).astype(np.float64) * scale.astype(np.float64) + (b * cb * scale).astype(np.float64)).astype(F)
    else:
        t = a * ca * scale + b * cb * scale
    if "desc_left_assoc" in mut:
        return base + a * ca * scale + b * cb * scale
    return base + t


def mldb_values(lt, lx, ly, kps, angle, channels, sampling, cov=None, pattern_size=10, mut=(), level_octave=None):
    """mldb_fill_values for the three grids: [29 cells, 3, n] float32 means (di, dx, dy; unused channels zero)."""
    mut = _check(mut)
    n = len(kps)
    h, w = lt.shape
    cov = cov or Coverage(n)
    smp = _Sampler(w, h, sampling, cov)
    ltf, lxf, lyf = (np.ascontiguousarray(a, F).ravel() for a in (lt, lx, ly))
    cells = []
    half = F(0.0) if "desc_no_half" in mut else F(0.5)
    with np.errstate(all="ignore"):
        ratio = _ratio(kps["octave"])  # the KEYPOINT's octave (descriptors.rs:51)
        if "desc_level_octave" in mut:
            ratio = _ratio(np.full(n, level_octave))
        scale = F(0.5) * kps["size"].astype(F) / ratio
        scale = np.trunc(scale) if "desc_scale_trunc" in mut else round_f32(scale, mut)
        xf, yf = kps["x"].astype(F) / ratio, kps["y"].astype(F) / ratio
        co, si = cosf(angle), sinf(angle)
        if "desc_rot_sign" in mut:
            si = -si
        for grid, mult in enumerate((F(1.0), F(2.0) / F(3.0), F(1.0) / F(2.0))):
            step = int((np.floor if "desc_step_floor" in mut else np.ceil)(F(pattern_size) * mult))
            origins = [(i, j) for i in range(-pattern_size, pattern_size, step) for j in range(-pattern_size, pattern_size, step)]
            if "desc_cells_j_outer" in mut:
                origins = [(i, j) for j in range(-pattern_size, pattern_size, step) for i in range(-pattern_size, pattern_size, step)]
            for i, j in origins[:(grid + 2) ** 2]:  # (mldb_binary_comparisons reads val_count cells: all of them, unless mutated)
                di, dx, dy = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
                nsamples = 0
                samples = [(k, l) for k in range(i, i + step) for l in range(j, j + step)]
                if "desc_kl_swapped" in mut:
                    samples = [(k, l) for l in range(j, j + step) for k in range(i, i + step)]
                for k, l in samples:
                    lf, kf = F(l) + half, F(k) + half
                    sample_y = _lattice(yf, lf, co, kf, si, scale, mut)
                    sample_x = _lattice(xf, -lf, si, kf, co, scale, mut)
                    p = smp.index(round_f32(sample_x, mut), round_f32(sample_y, mut), False)
                    di = di + ltf[p]
                    if channels > 1:
                        rx, ry = lxf[p], lyf[p]
                        if channels == 2:
                            if "desc_sqrt_f64" in mut:
                                dx = dx + np.hypot(rx.astype(np.float64), ry.astype(np.float64)).astype(F)
                            else:
                                dx = dx + np.sqrt(rx * rx + ry * ry)
                        else:
                            rry = rx * co + ry * si
                            rrx = -rx * si + ry * co
                            if "desc_dxdy_swapped" in mut:
                                rrx, rry = rry, rrx
                            dx = dx + rrx
                            dy = dy + rry
                    nsamples += 1
                ns = F(nsamples)
                if "desc_no_div" in mut:
                    cells.append((di, dx, dy))
                elif "desc_recip" in mut:
                    cells.append((di * (F(1.0) / ns), dx * (F(1.0) / ns), dy * (F(1.0) / ns)))
                else:
                    cells.append((di / ns, dx / ns, dy / ns))
    assert len(cells) == 29
    return np.array(cells, F)


def mldb_bits(values, channels, mut=()):
    """mldb_binary_comparisons over the three grids: [n, ceil(162 * channels / 8)] bytes, bits LSB first."""
    mut = _check(mut)
    n = values.shape[2]
    bits = []
    base = 0
    for count in (4, 9, 16):
        triples = [(pos, i, j) for pos in range(channels) for i in range(count) for j in range(i + 1, count)]
        if "desc_channel_minor" in mut:
            triples = [(pos, i, j) for i in range(count) for j in range(i + 1, count) for pos in range(channels)]
        for pos, i, j in triples:
            with np.errstate(invalid="ignore"):
                if "desc_ge" in mut:
                    bits.append(values[base + i, pos] >= values[base + j, pos])
                else:
                    bits.append(values[base + i, pos] > values[base + j, pos])
        base += count
    bits = np.array(bits, np.uint8).T.reshape(n, -1)
    assert bits.shape[1] == 162 * channels
    return np.packbits(bits, axis=1, bitorder="big" if "desc_msb_first" in mut else "little")


def describe_level(lt, lx, ly, level_octave, kps, channels, sampling, compute_orientation=True, mut=()):
    """Both ops on keypoints of one level.  Returns (angles float32[n], descriptors uint8[n, bytes], Coverage)."""
    mut = _check(mut)
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    cov = Coverage(len(kps))
    angle = kps["angle"].astype(F)
    if compute_orientation:
        angle = main_orientation(lx, ly, level_octave, kps, sampling, cov, mut)
    values = mldb_values(lt, lx, ly, kps, angle, channels, sampling, cov, mut=mut, level_octave=level_octave)
    return angle, mldb_bits(values, channels, mut), cov


def describe(planes, octaves, kps, channels, sampling, compute_orientation=True, mut=()):
    """describe_level over a keypoint list that mixes levels: planes[level] = (Lt, Lx, Ly), octaves[level] = the level's
    octave; class_id picks the level.  Rows come back in the order of `kps`."""
    mut = _check(mut)
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    n = len(kps)
    angle = np.zeros(n, F)
    desc = np.zeros((n, (162 * channels + 7) // 8), np.uint8)
    cov = Coverage(n)
    for lvl in np.unique(kps["class_id"]):
        sel = np.nonzero(kps["class_id"] == lvl)[0]
        lt, lx, ly = planes[int(lvl)]
        a, d, c = describe_level(lt, lx, ly, octaves[int(lvl)], kps[sel], channels, sampling, compute_orientation, mut)
        angle[sel], desc[sel] = a, d
        for f in ("left", "right", "top", "bottom", "next_row", "completes"):
            getattr(cov, f)[sel] = getattr(c, f)
    return angle, desc, cov
