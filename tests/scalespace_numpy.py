"""A plain numpy / Python statement of the front half of AKAZE, from the frame to Ldet -- the image filters
(akaze/src/types/image.rs:102-118, :239-380), the Scharr derivatives (ops/derivatives.rs:41-130), pm_g2 and
create_nonlinear_scale_space (lib.rs:26-120), compute_contrast_factor (ops/contrast_factor.rs:18-71), calculate_step
(ops/nonlinear_diffusion.rs:15-173), the FED schedule (ops/fed_tau.rs:27-106), allocate_evolutions (types/evolution.rs:101-161)
and detector_response (ops/detector_response.rs:8-55) -- written from the reference's text, independently of the oracle
(oracle/akaze_ref.cpp) and of the product's kernels and host code.  It imports neither.  TEST INFRASTRUCTURE ONLY.

float32 throughout except where the reference works in f64 (pm_g2, the contrast factor, the Scharr norm, the level plan and
the FED schedule, which are Python floats here).  numpy rounds every float32 operation on its own and fuses nothing, so an
expression written in the reference's order gives the reference's bits.  The filters work on the FLAT buffer as the reference
does: a tap's products are added over one flat range, rows wrapping into each other, and fill_border then overwrites what the
wrap touched.  expf is the process's libm through ctypes (np.exp on float32 may differ in the last bit); math.cos and `**` on
Python floats are the same glibc the reference's f64::cos / f64::powf bind to.

Chained with tests/extrema_numpy.py (detection on Ldet) and tests/mldb_numpy.py (orientation and M-LDB on Lt, Lx, Ly) this is
a whole AKAZE from the frame to the descriptor bytes that shares no code with the oracle or the product.

MUTATIONS.  Every function takes `mut`, a collection of switch names; each switch flips ONE rule of the statement.  They exist
only so that tests/test_scalespace_host.py can prove that the inputs of tests/scalespace_cases.py tell the right statement from
a wrong one; nothing else may pass a switch.

  half_row_major             half_size adds (x, y), (x+1, y), (x, y+1), (x+1, y+1): rows outer (image.rs:109-110)
  pm_g2_f32                  pm_g2 in f32 (lib.rs:30-37)
  tau_f64                    the step scaled by the f64 tau, in f64, and rounded once (nonlinear_diffusion.rs:67)
  fed_sum_order              (x_pos + y_pos) - (x_neg + y_neg) in the interior (:67)
  fed_border_zero_terms      the border expressions (:84-137) as the interior one with +0.0 for each missing term: other
                             WORDS only (the sign of a zero), never other values
  contrast_whole_image       border pixels take part in the maximum and the histogram (contrast_factor.rs:30-31, :40-41)
  contrast_zero_counted      pixels with modg == 0 are counted (:45)
  contrast_no_clamp_guard    bin_number == num_bins is not taken down (:47-49): those pixels count as points, in no bin
  contrast_thr_le            `num_elements <= threshold` in the walk (:58)
  k_not_scaled_per_octave    no `contrast_factor *= 0.75` at an octave change (lib.rs:84)
  lt_from_level0             every level's Lt starts from level 0's Lt, not from the diffused Lt before it (lib.rs:82, :92)
  lsmooth0_blurred           level 0's Lsmooth is gaussian_blur(Lt, 1.0), not the clone of lib.rs:58
  scharr_vertical_pass_first the vertical pass of the separable Scharr before the horizontal one (derivatives.rs:45-46, :63-64)
  taps_reversed              the taps of both filters accumulated from +hw down to -hw (image.rs:280, :315)
  lxy_from_ly                Lxy = scharr(Ly, x) instead of scharr(Lx, y) (detector_response.rs:13)
  lx_ly_of_flow_kept         the sigma-1 Lx / Ly of lib.rs:98-103 stay; the detector's (detector_response.rs:9-10) are dropped
  sigma_round_half_even      the detector's sigma_size by banker's rounding (detector_response.rs:24, :42)
  ldet_quat_last_f64         the determinant formed AND scaled in f64, rounded once (detector_response.rs:52).  (Only the
                             multiplication by sigma_size^4 in f64 changes nothing: the f64 product of two f32 values is
                             exact, so rounding it gives the f32 product.)
  blur_size_round            the Gaussian kernel size from round(r), not ceil(r) (image.rs:376)

Not switches, because they give the same bits on every input: `val / 4` against `val * 0.25` in half_size (a division by a
power of two is exact wherever the product is), and `0.5 * tau` taken first or last in calculate_step (0.5 * x is exact down
to the last subnormal bit only when taken first -- the reference takes it first, :67, and so does this statement).

INVISIBLE, two more switches that change nothing (tests/test_scalespace_host.py shows it on every filter shape): the flat
loops of the filters stop ONE pixel early (image.rs:286, :323) and the horizontal one wraps rows into each other; fill_border
overwrites every pixel either touches.  `filter_full_range` runs the loops to the end, `filter_no_wrap` zeroes what the wrap
wrote.  They are here so that nobody "fixes" one side only.  (With a ONE-tap kernel fill_border fills nothing and the
unprocessed last pixel stays 0; every kernel in use has three taps or more.)
"""
import ctypes as C
import ctypes.util
import math

import numpy as np

F = np.float32
PLANES = ["Lt", "Lsmooth", "Lx", "Ly", "Lxx", "Lyy", "Lxy", "Lflow", "Lstep", "Ldet"]
SWITCHES = ("half_row_major", "pm_g2_f32", "tau_f64", "fed_sum_order", "fed_border_zero_terms", "contrast_whole_image",
            "contrast_zero_counted", "contrast_no_clamp_guard", "contrast_thr_le", "k_not_scaled_per_octave", "lt_from_level0",
            "lsmooth0_blurred", "scharr_vertical_pass_first", "taps_reversed", "lxy_from_ly", "lx_ly_of_flow_kept",
            "sigma_round_half_even", "ldet_quat_last_f64", "blur_size_round")
INVISIBLE = ("filter_full_range", "filter_no_wrap")
USIZE_MAX = (1 << 64) - 1

_expf = None


def _check(mut):
    bad = set(mut) - set(SWITCHES) - set(INVISIBLE)
    assert not bad, bad
    return frozenset(mut)


def expf(x):
    """the process's expf (glibc), one float32 in, one out"""
    global _expf
    if _expf is None:
        m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        m.expf.argtypes, m.expf.restype = [C.c_float], C.c_float
        _expf = m.expf
    return F(_expf(float(F(x))))


def unit_float(u8):
    """create_unit_float_image (image.rs:136): f32::from(v) * 1f32 / 255f32"""
    return (np.asarray(u8).astype(F) * F(1.0)) / F(255.0)


# ---- types/image.rs ---------------------------------------------------------------------------------------------------------
def filter_fits(w, h, klen):
    """the shapes on which both filters run to the end in the reference (no index past the buffer, :283-284, :318-321, and
    fill_border's columns / rows hw and size - hw - 1 exist, :241-242, :251-252)"""
    return min(w, h) >= 2 * (klen // 2) + 1


def fill_border(out, hw):
    """:239-260 in place on a 2-D array: rows first, then columns; a column's (row's) two sources are read before its writes"""
    h, w = out.shape
    plus, minus = out[hw, :].copy(), out[h - hw - 1, :].copy()
    out[:hw, :] = plus
    out[h - hw:, :] = minus
    plus, minus = out[:, hw].copy(), out[:, w - hw - 1].copy()
    out[:, :hw] = plus[:, None]
    out[:, w - hw:] = minus[:, None]


def _filter(img, kernel, stride_rows, mut):
    img = np.ascontiguousarray(img, F)
    kernel = np.ascontiguousarray(kernel, F)
    assert len(kernel) % 2 == 1  # :272
    h, w = img.shape
    hw = len(kernel) // 2
    assert filter_fits(w, h, len(kernel)), (w, h, len(kernel))
    src = img.ravel()
    out = np.zeros(w * h, F)  # the output starts at zero (:276)
    unit = w if stride_rows else 1
    lo, hi = hw * unit, w * h - hw * unit - 1  # :286 / :323
    if "filter_full_range" in mut:
        hi += 1
    ks = range(hw, -hw - 1, -1) if "taps_reversed" in mut else range(-hw, hw + 1)
    for k in ks:  # one tap after another over the whole flat range (:280-291)
        out[lo:hi] += kernel[k + hw] * src[lo + k * unit:hi + k * unit]
    out = out.reshape(h, w)
    if "filter_no_wrap" in mut and not stride_rows:
        out[:, :hw] = 0
        out[:, w - hw:] = 0
    fill_border(out, hw)
    return out


def horizontal_filter(img, kernel, mut=()):
    """:270-295"""
    return _filter(img, kernel, False, _check(mut))


def vertical_filter(img, kernel, mut=()):
    """:305-332"""
    return _filter(img, kernel, True, _check(mut))


def gaussian(x, r):
    """:341-343: ((2 pi).sqrt() * r).recip() * (-x^2 / (2 r^2)).exp(), every operation in f32"""
    x, r = F(x), F(r)
    a = F(1.0) / (np.sqrt(F(2.0) * F(np.pi)) * r)
    return a * expf(-(x * x) / (F(2.0) * (r * r)))


def gaussian_kernel(r, kernel_size):
    """:352-365: the sum is sequential in f32"""
    hw = kernel_size // 2
    kernel = np.zeros(kernel_size, F)
    total = F(0.0)
    for i in range(-hw, hw + 1):
        val = gaussian(F(i), r)
        kernel[i + hw] = val
        total = F(total + val)
    return kernel / total


def gaussian_kernel_size(r, mut=()):
    """:376: ceil(r) * 2 + 1"""
    r = float(F(r))
    n = math.floor(r + 0.5) if "blur_size_round" in _check(mut) else math.ceil(r)
    return int(n) * 2 + 1


def gaussian_blur(img, r, mut=()):
    """:374-380"""
    kernel = gaussian_kernel(F(r), gaussian_kernel_size(r, mut))
    return vertical_filter(horizontal_filter(img, kernel, mut), kernel, mut)


def half_size(img, mut=()):
    """:102-118: val = 0; the source column outer, the source row inner; val / 4"""
    mut = _check(mut)
    img = np.ascontiguousarray(img, F)
    h, w = img.shape[0] // 2, img.shape[1] // 2
    p = lambda dx, dy: img[dy:2 * h:2, dx:2 * w:2]
    order = ((0, 0), (1, 0), (0, 1), (1, 1)) if "half_row_major" in mut else ((0, 0), (0, 1), (1, 0), (1, 1))
    val = np.zeros((h, w), F)
    for dx, dy in order:
        val = val + p(dx, dy)
    return val / F(4.0)


# ---- ops/derivatives.rs -----------------------------------------------------------------------------------------------------
def scharr_kernels(scale):
    """:74-101: (main axis, off axis); the norm in f64, each tap rounded on its own"""
    size = 3 + 2 * (scale - 1)
    w = 10.0 / 3.0
    norm = 1.0 / (2.0 * float(scale) * (w + 2.0))
    main, off = np.zeros(size, F), np.zeros(size, F)
    main[0], main[size // 2], main[size - 1] = F(norm), F(w * norm), F(norm)
    off[0], off[size // 2], off[size - 1] = F(-1.0), F(0.0), F(1.0)
    return main, off


def _separable(img, k_horizontal, k_vertical, mut):
    if "scharr_vertical_pass_first" in mut:
        return horizontal_filter(vertical_filter(img, k_vertical, mut), k_horizontal, mut)
    return vertical_filter(horizontal_filter(img, k_horizontal, mut), k_vertical, mut)


def scharr(img, x_order, y_order, sigma_size, mut=()):
    """:41-65, :112-130.  scharr_horizontal filters rows with the main-axis kernel and columns with the off-axis one,
    scharr_vertical the other way round; both orders: scharr_horizontal twice, added (sqrt_squared only adds, image.rs:218-231);
    neither: zeros."""
    mut = _check(mut)
    img = np.ascontiguousarray(img, F)
    if not (x_order or y_order):
        return np.zeros(img.shape, F)
    main, off = scharr_kernels(int(sigma_size))
    if x_order and y_order:
        horizontal = _separable(img, main, off, mut)
        vertical = _separable(img, main, off, mut)
        return vertical + horizontal
    if x_order:
        return _separable(img, main, off, mut)
    return _separable(img, off, main, mut)


# ---- lib.rs:26-41 -----------------------------------------------------------------------------------------------------------
def pm_g2(lx, ly, k, mut=()):
    """1 / (1 + (1 / k^2) (Lx^2 + Ly^2)) in f64, one rounding to f32 at the end"""
    mut = _check(mut)
    with np.errstate(all="ignore"):
        if "pm_g2_f32" in mut:
            lx, ly, k = np.asarray(lx, F), np.asarray(ly, F), F(k)
            inverse_k = F(1.0) / (k * k)
            return (F(1.0) / (F(1.0) + inverse_k * (lx * lx + ly * ly))).astype(F)
        lx, ly, k = np.asarray(lx, F).astype(np.float64), np.asarray(ly, F).astype(np.float64), np.float64(k)
        inverse_k = np.float64(1.0) / (k * k)
        return (1.0 / (1.0 + inverse_k * (lx * lx + ly * ly))).astype(F)


# ---- ops/contrast_factor.rs -------------------------------------------------------------------------------------------------
def as_usize(v):
    """Rust's f64 `as usize`: truncating, saturating, NaN and negatives to 0"""
    if not (v > 0.0):
        return 0
    if v >= 18446744073709551615.0:
        return USIZE_MAX
    return int(v)


def compute_contrast_factor(img, percentile, gradient_histogram_scale, num_bins, mut=()):
    """:18-71.  Interior pixels only, all arithmetic f64, a pixel counts if modg != 0 (a NaN does), the bin that equals
    num_bins is taken down by one, the threshold truncates, 0.03 if the walk ends below it."""
    mut = _check(mut)
    num_bins = int(num_bins)
    blurred = gaussian_blur(img, F(gradient_histogram_scale), mut)
    lx = scharr(blurred, True, False, 1, mut).astype(np.float64)
    ly = scharr(blurred, False, True, 1, mut).astype(np.float64)
    if "contrast_whole_image" not in mut:
        lx, ly = lx[1:-1, 1:-1], ly[1:-1, 1:-1]
    with np.errstate(all="ignore"):
        modg = np.sqrt(lx * lx + ly * ly).ravel()
        hmax = 0.0
        if modg.size and (modg > 0.0).any():  # `if modg > hmax` from 0.0: a NaN never replaces the maximum
            hmax = float(np.nanmax(modg))
        counted = modg if "contrast_zero_counted" in mut else modg[modg != 0.0]
        q = np.floor(float(num_bins) * (counted / hmax))
    bins = np.where(np.isnan(q), 0.0, np.clip(q, 0.0, float(num_bins))).astype(np.int64)  # `as usize`
    if "contrast_no_clamp_guard" not in mut:
        bins = np.where(bins == num_bins, num_bins - 1, bins)
    histogram = np.bincount(bins, minlength=num_bins + 1)[:num_bins]
    num_points = float(len(counted))
    threshold = as_usize(num_points * percentile)
    k = num_elements = 0
    while (num_elements <= threshold if "contrast_thr_le" in mut else num_elements < threshold) and k < num_bins:
        num_elements += int(histogram[k])
        k += 1
    if num_elements >= threshold:
        return hmax * float(k) / float(num_bins)
    return 0.03


# ---- ops/nonlinear_diffusion.rs ---------------------------------------------------------------------------------------------
def calculate_step(lt, lflow, tau, mut=()):
    """:15-144: (Lt + Lstep, Lstep).  A flux is (c_a + c_b) * (L_p - L_q) (eval, :149-173); the interior adds
    x_pos - x_neg + y_pos - y_neg from the left (:67), the eight border expressions leave out the terms that would look
    outside (:84-137), and the last row's y_pos reads [0, -1, -1, 0]: (c[y] + c[y-1]) * (L[y-1] - L[y]) (:106, :112, :116)."""
    mut = _check(mut)
    L, c = np.ascontiguousarray(lt, F), np.ascontiguousarray(lflow, F)
    h, w = L.shape
    assert h >= 2 and w >= 2
    with np.errstate(all="ignore"):
        # fluxes of pixel (x, y) for every pixel that has the neighbour
        x_pos = (c[:, :-1] + c[:, 1:]) * (L[:, 1:] - L[:, :-1])   # pixel x = 0 .. w-2 at column x
        x_neg = x_pos   # pixel x = 1 .. w-1 at column x - 1: (c[x-1] + c[x]) * (L[x] - L[x-1]), the same operands
        y_pos = (c[:-1, :] + c[1:, :]) * (L[1:, :] - L[:-1, :])   # pixel y = 0 .. h-2 at row y
        y_neg = y_pos   # pixel y = 1 .. h-1 at row y - 1
        y_last = (c[h - 1, :] + c[h - 2, :]) * (L[h - 2, :] - L[h - 1, :])  # the last row's y_pos
        s = np.zeros((h, w), F)
        Z = F(0.0)
        zt = "fed_border_zero_terms" in mut
        # interior (:30-81)
        xp, xn, yp, yn = x_pos[1:-1, 1:], x_neg[1:-1, :-1], y_pos[1:, 1:-1], y_neg[:-1, 1:-1]
        s[1:-1, 1:-1] = ((xp + yp) - (xn + yn)) if "fed_sum_order" in mut else (xp - xn + yp - yn)
        # first row (:83-102)
        xp, xn, yp = x_pos[0, 1:], x_neg[0, :-1], y_pos[0, 1:-1]
        s[0, 1:-1] = (xp - xn + yp - Z) if zt else (xp - xn + yp)
        s[0, 0] = (x_pos[0, 0] - Z + y_pos[0, 0] - Z) if zt else (x_pos[0, 0] + y_pos[0, 0])
        s[0, w - 1] = (Z - x_neg[0, w - 2] + y_pos[0, w - 1] - Z) if zt else (-x_neg[0, w - 2] + y_pos[0, w - 1])
        # last row (:104-119)
        xp, xn, yp = x_pos[h - 1, 1:], x_neg[h - 1, :-1], y_last[1:-1]
        s[h - 1, 1:-1] = (xp - xn + yp - Z) if zt else (xp - xn + yp)
        s[h - 1, 0] = (x_pos[h - 1, 0] - Z + y_last[0] - Z) if zt else (x_pos[h - 1, 0] + y_last[0])
        s[h - 1, w - 1] = (Z - x_neg[h - 1, w - 2] + y_last[w - 1] - Z) if zt else (-x_neg[h - 1, w - 2] + y_last[w - 1])
        # first and last columns (:121-138)
        xp, yp, yn = x_pos[1:-1, 0], y_pos[1:, 0], y_neg[:-1, 0]
        s[1:-1, 0] = (xp - Z + yp - yn) if zt else (xp + yp - yn)
        xn, yp, yn = x_neg[1:-1, w - 2], y_pos[1:, w - 1], y_neg[:-1, w - 1]
        s[1:-1, w - 1] = (Z - xn + yp - yn) if zt else (-xn + yp - yn)
        if "tau_f64" in mut:
            lstep = (0.5 * float(tau) * s.astype(np.float64)).astype(F)
        else:
            lstep = (F(0.5) * F(tau)) * s  # 0.5 * (step_size as f32) * (...)
        return L + lstep, lstep  # :140-143


# ---- ops/fed_tau.rs ---------------------------------------------------------------------------------------------------------
def _is_prime(n):
    return n >= 2 and all(n % d for d in range(2, int(math.isqrt(n)) + 1))


def fed_tau_by_process_time(T, M=1, tau_max=0.25, reordering=True):
    """:27-106 in Python floats (f64).  n == 1 with reordering never ends in the reference (:95-99: kappa is 0 and the index
    wraps below zero): ValueError."""
    t = T / float(M)
    n = as_usize(math.ceil(math.sqrt(3.0 * t / tau_max + 0.25) - 0.5 - 1.0e-8) + 0.5)  # :45
    if n == 0:
        return np.zeros(0, np.float64)
    scale = 3.0 * t / (tau_max * float(n * (n + 1)))
    c = 1.0 / (4.0 * float(n) + 2.0)
    d = scale * tau_max / 2.0
    tauh = []
    for k in range(n):
        hh = math.cos(math.pi * (2.0 * float(k) + 1.0) * c)
        tauh.append(d / (hh * hh))
    if not reordering:
        return np.array(tauh, np.float64)
    if n == 1:
        raise ValueError("fed_tau: the reordering of a one-step schedule does not terminate")
    kappa = n // 2
    prime = n + 1
    while not _is_prime(prime):
        prime += 1
    tau, k = [], 0
    for _ in range(n):
        index = ((k + 1) * kappa) % prime - 1  # (usize: -1 wraps to the largest value, which is >= n)
        while index >= n or index < 0:
            k += 1
            index = ((k + 1) * kappa) % prime - 1
        tau.append(tauh[index])
        k += 1
    return np.array(tau, np.float64)


# ---- types/evolution.rs -----------------------------------------------------------------------------------------------------
def round_half_away(x):
    """f64::round"""
    t = float(math.trunc(x))
    return t + math.copysign(1.0, x) if abs(x - t) >= 0.5 else t


def allocate_evolutions(width, height, cfg):
    """:101-161: [dict(etime, esigma, octave, sublevel, sigma_size, tau)]; level 0 has no steps"""
    out = []
    for i in range(int(cfg.max_octave_evolution)):
        rfactor = 1.0 / 2.0 ** float(i)
        level_height, level_width = int(float(height) * rfactor), int(float(width) * rfactor)
        if not ((level_width >= 80 and level_height >= 40) or i == 0):
            break
        for j in range(int(cfg.num_sublevels)):
            esigma = float(cfg.base_scale_offset) * 2.0 ** (float(j) / float(cfg.num_sublevels) + float(i))
            out.append(dict(etime=0.5 * (esigma * esigma), esigma=esigma, octave=i, sublevel=j,
                            sigma_size=int(round_half_away(esigma)), tau=np.zeros(0, np.float64)))
    for i in range(1, len(out)):
        out[i]["tau"] = fed_tau_by_process_time(out[i]["etime"] - out[i - 1]["etime"], 1, 0.25, True)
    return out


# ---- ops/detector_response.rs -----------------------------------------------------------------------------------------------
def detector_sigma(esigma, octave, derivative_factor, mut=()):
    """:22-24, :41-42: f64::round(esigma * derivative_factor / 2^octave) as u32"""
    v = float(esigma) * float(derivative_factor) / 2.0 ** float(octave)
    return int(round(v)) if "sigma_round_half_even" in _check(mut) else int(round_half_away(v))


def detector_response(lsmooth, sigma_size, mut=()):
    """:8-14, :43-52 for one level: {Lx, Ly, Lxx, Lyy, Lxy, Ldet}"""
    mut = _check(mut)
    s = int(sigma_size)
    lx = scharr(lsmooth, True, False, s, mut)
    ly = scharr(lsmooth, False, True, s, mut)
    lxx = scharr(lx, True, False, s, mut)
    lyy = scharr(ly, False, True, s, mut)
    lxy = scharr(ly, True, False, s, mut) if "lxy_from_ly" in mut else scharr(lx, False, True, s, mut)
    quat = s * s * s * s
    with np.errstate(all="ignore"):
        if "ldet_quat_last_f64" in mut:
            a, b, c = lxx.astype(np.float64), lyy.astype(np.float64), lxy.astype(np.float64)
            ldet = (((a * b) - (c * c)) * float(quat)).astype(F)
        else:
            ldet = ((lxx * lyy) - (lxy * lxy)) * F(quat)
    return dict(Lx=lx, Ly=ly, Lxx=lxx, Lyy=lyy, Lxy=lxy, Ldet=ldet)


# ---- lib.rs:49-138 ----------------------------------------------------------------------------------------------------------
def pyramid(frame, cfg, mut=()):
    """create_nonlinear_scale_space + detector_response on a u8 frame (converted as create_unit_float_image does) or an f32
    one; cfg is anything with Config's attributes.  Returns (levels, contrast factor): a level is a dict of the info fields
    (etime, esigma, octave, sublevel, sigma_size, w, h), `tau` and `planes`, the ten planes by name.  Level 0 has no Lflow and
    no Lstep: (0, 0) arrays."""
    mut = _check(mut)
    frame = np.asarray(frame)
    image = unit_float(frame) if frame.dtype == np.uint8 else np.ascontiguousarray(frame, F)
    h, w = image.shape
    levels = allocate_evolutions(w, h, cfg)
    empty = lambda: np.zeros((0, 0), F)
    lt = gaussian_blur(image, F(float(cfg.base_scale_offset)), mut)  # `options.base_scale_offset as f32`
    lt0 = lt
    levels[0]["planes"] = dict(Lt=lt, Lsmooth=gaussian_blur(lt, F(1.0), mut) if "lsmooth0_blurred" in mut else lt.copy(),
                               Lflow=empty(), Lstep=empty())
    contrast = compute_contrast_factor(lt, float(cfg.contrast_percentile), 1.0, int(cfg.contrast_factor_num_bins), mut)
    k = contrast
    for i in range(1, len(levels)):
        new_octave = levels[i]["octave"] > levels[i - 1]["octave"]
        if "lt_from_level0" in mut:
            lt = lt0
            for _ in range(levels[i]["octave"]):
                lt = half_size(lt, mut)
        elif new_octave:
            lt = half_size(lt, mut)
        if new_octave and "k_not_scaled_per_octave" not in mut:
            k = k * 0.75
        lsmooth = gaussian_blur(lt, F(1.0), mut)
        lx, ly = scharr(lsmooth, True, False, 1, mut), scharr(lsmooth, False, True, 1, mut)
        lflow = pm_g2(lx, ly, k, mut)
        lstep = np.zeros(lt.shape, F)
        for tau in levels[i]["tau"]:
            lt, lstep = calculate_step(lt, lflow, tau, mut)
        levels[i]["planes"] = dict(Lt=lt, Lsmooth=lsmooth, Lflow=lflow, Lstep=lstep, Lx=lx, Ly=ly)
    for i, lv in enumerate(levels):
        p = lv["planes"]
        lv["h"], lv["w"] = p["Lt"].shape
        det = detector_response(p["Lsmooth"], detector_sigma(lv["esigma"], lv["octave"], cfg.derivative_factor, mut), mut)
        if "lx_ly_of_flow_kept" in mut and i > 0:
            det["Lx"], det["Ly"] = p["Lx"], p["Ly"]
        p.update(det)
    return levels, contrast


def extract(frame, cfg, mut=()):
    """The whole chain: pyramid() -> tests/extrema_numpy.py detect on its Ldet -> tests/mldb_numpy.py describe on its Lt, Lx and
    Ly (the reference's own sampling; every sample must stay inside its plane).  Returns (keypoints with their angles,
    descriptor rows, levels, contrast factor)."""
    import extrema_numpy as E
    import mldb_numpy as M
    levels, contrast = pyramid(frame, cfg, mut)
    lv = [(l["w"], l["h"], l["octave"], l["esigma"]) for l in levels]
    kps, _ = E.detect([l["planes"]["Ldet"] for l in levels], lv, cfg)
    planes = [tuple(l["planes"][p] for p in ("Lt", "Lx", "Ly")) for l in levels]
    angle, desc, cov = M.describe(planes, [l["octave"] for l in levels], kps, int(cfg.descriptor_channels), "reference")
    assert cov.completes.all() and not cov.next_row.any()
    kps["angle"] = angle
    return kps, desc, levels, contrast
