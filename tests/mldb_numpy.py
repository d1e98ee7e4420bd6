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


def round_f32(x):
    """f32::round: to the nearest integer, halves away from zero; NaN and the infinities pass through."""
    x = np.asarray(x, F)
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


def orientation_windows():
    """the (ang1, ang2) of every window of scale_space_extrema.rs:300-310, ang1 already advanced (it is, before the test)"""
    out = []
    ang1 = F(0)
    while ang1 < F(2.0) * PI:
        ang2 = ang1 - F(5.0) * PI / F(3.0) if ang1 + PI / F(3.0) > F(2.0) * PI else ang1 + PI / F(3.0)
        ang1 = F(ang1 + F(0.15))
        out.append((ang1, F(ang2)))
    return out


def main_orientation(lx, ly, level_octave, kps, sampling, cov=None):
    """compute_main_orientation for keypoints of ONE level (its Lx, Ly as 2-D float32 arrays, its octave): the angle of
    every keypoint, the given one where no window's vector is longer than zero."""
    n = len(kps)
    h, w = lx.shape
    cov = cov or Coverage(n)
    smp = _Sampler(w, h, sampling, cov)
    lxf, lyf = np.ascontiguousarray(lx, F).ravel(), np.ascontiguousarray(ly, F).ravel()
    with np.errstate(all="ignore"):
        ratio = _ratio(np.full(n, level_octave))  # the LEVEL's octave (:279), not the keypoint's
        s = round_f32(F(0.5) * kps["size"].astype(F) / ratio)
        xf, yf = kps["x"].astype(F) / ratio, kps["y"].astype(F) / ratio
        ident = [6, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6]
        res_x, res_y = [], []
        for i in range(-6, 7):
            for j in range(-6, 7):
                if i * i + j * j < 36:
                    fy = round_f32(yf + F(j) * s)
                    fx = round_f32(xf + F(i) * s)
                    p = smp.index(fx, fy, True)
                    g = GAUSS25[ident[i + 6]][ident[j + 6]]
                    res_x.append(g * lxf[p])
                    res_y.append(g * lyf[p])
        assert len(res_x) == 109
        res_x, res_y = np.array(res_x, F), np.array(res_y, F)  # [109, n]
        angs = atan2f(res_y, res_y)                              # (:294: res_y twice)
        sum_x, sum_y, best = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
        bx, by, found = np.zeros(n, F), np.zeros(n, F), np.zeros(n, bool)
        two_pi = F(2.0) * PI
        for ang1, ang2 in orientation_windows():
            for k in range(109):
                ang = angs[k]
                if ang1 < ang2:
                    take = (ang1 < ang) & (ang < ang2)
                elif ang2 < ang1:
                    take = ((ang > F(0)) & (ang < ang2)) | ((ang > ang1) & (ang < two_pi))
                else:
                    take = np.zeros(n, bool)
                sum_x = np.where(take, sum_x + res_x[k], sum_x)
                sum_y = np.where(take, sum_y + res_y[k], sum_y)
            val = sum_x * sum_x + sum_y * sum_y
            new = val > best
            best = np.where(new, val, best)
            bx, by = np.where(new, sum_x, bx), np.where(new, sum_y, by)
            found |= new
        return np.where(found, atan2f(by, bx), kps["angle"].astype(F)).astype(F)


def mldb_values(lt, lx, ly, kps, angle, channels, sampling, cov=None, pattern_size=10):
    """mldb_fill_values for the three grids: [29 cells, 3, n] float32 means (di, dx, dy; unused channels zero)."""
    n = len(kps)
    h, w = lt.shape
    cov = cov or Coverage(n)
    smp = _Sampler(w, h, sampling, cov)
    ltf, lxf, lyf = (np.ascontiguousarray(a, F).ravel() for a in (lt, lx, ly))
    cells = []
    with np.errstate(all="ignore"):
        ratio = _ratio(kps["octave"])  # the KEYPOINT's octave (descriptors.rs:51)
        scale = round_f32(F(0.5) * kps["size"].astype(F) / ratio)
        xf, yf = kps["x"].astype(F) / ratio, kps["y"].astype(F) / ratio
        co, si = cosf(angle), sinf(angle)
        for mult in (F(1.0), F(2.0) / F(3.0), F(1.0) / F(2.0)):
            step = int(np.ceil(F(pattern_size) * mult))
            for i in range(-pattern_size, pattern_size, step):
                for j in range(-pattern_size, pattern_size, step):
                    di, dx, dy = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
                    nsamples = 0
                    for k in range(i, i + step):
                        for l in range(j, j + step):
                            lf, kf = F(l) + F(0.5), F(k) + F(0.5)
                            sample_y = yf + (lf * co * scale + kf * si * scale)
                            sample_x = xf + (-lf * si * scale + kf * co * scale)
                            p = smp.index(round_f32(sample_x), round_f32(sample_y), False)
                            di = di + ltf[p]
                            if channels > 1:
                                rx, ry = lxf[p], lyf[p]
                                if channels == 2:
                                    dx = dx + np.sqrt(rx * rx + ry * ry)
                                else:
                                    rry = rx * co + ry * si
                                    rrx = -rx * si + ry * co
                                    dx = dx + rrx
                                    dy = dy + rry
                            nsamples += 1
                    ns = F(nsamples)
                    cells.append((di / ns, dx / ns, dy / ns))
    assert len(cells) == 29
    return np.array(cells, F)


def mldb_bits(values, channels):
    """mldb_binary_comparisons over the three grids: [n, ceil(162 * channels / 8)] bytes, bits LSB first."""
    n = values.shape[2]
    bits = []
    base = 0
    for count in (4, 9, 16):
        for pos in range(channels):
            for i in range(count):
                for j in range(i + 1, count):
                    with np.errstate(invalid="ignore"):
                        bits.append(values[base + i, pos] > values[base + j, pos])
        base += count
    bits = np.array(bits, np.uint8).T.reshape(n, -1)
    assert bits.shape[1] == 162 * channels
    return np.packbits(bits, axis=1, bitorder="little")


def describe_level(lt, lx, ly, level_octave, kps, channels, sampling, compute_orientation=True):
    """Both ops on keypoints of one level.  Returns (angles float32[n], descriptors uint8[n, bytes], Coverage)."""
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    cov = Coverage(len(kps))
    angle = kps["angle"].astype(F)
    if compute_orientation:
        angle = main_orientation(lx, ly, level_octave, kps, sampling, cov)
    desc = mldb_bits(mldb_values(lt, lx, ly, kps, angle, channels, sampling, cov), channels)
    return angle, desc, cov


def describe(planes, octaves, kps, channels, sampling, compute_orientation=True):
    """describe_level over a keypoint list that mixes levels: planes[level] = (Lt, Lx, Ly), octaves[level] = the level's
    octave; class_id picks the level.  Rows come back in the order of `kps`."""
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    n = len(kps)
    angle = np.zeros(n, F)
    desc = np.zeros((n, (162 * channels + 7) // 8), np.uint8)
    cov = Coverage(n)
    for lvl in np.unique(kps["class_id"]):
        sel = np.nonzero(kps["class_id"] == lvl)[0]
        lt, lx, ly = planes[int(lvl)]
        a, d, c = describe_level(lt, lx, ly, octaves[int(lvl)], kps[sel], channels, sampling, compute_orientation)
        angle[sel], desc[sel] = a, d
        for f in ("left", "right", "top", "bottom", "next_row", "completes"):
            getattr(cov, f)[sel] = getattr(c, f)
    return angle, desc, cov
