"""Inputs that push the plane kernels and the extraction to the bottom and the top of f32, shared by
tests/test_numeric_range_host.py (the conditions below, asserted on the oracle alone) and tests/test_gpu_numeric_range.py.

Frames: the unit-range synthetic frame, optionally minus 0.5, times 2^e.  Two shapes, the smallest whose plan under the default
Config has three octaves (the third is admitted from 320 x 160 on, evolution.rs:138-149) with every level at least 16 px
each way: 320 x 160 (levels 320, 160 and 80 wide: a multiple of 8 in every octave) and 327 x 163 (163 x 81 and 81 x 40: odd).

Regimes, with what the oracle shows for them at detector_threshold = 0 (320 x 160 / 327 x 163; shares over all levels, the
conditions of REGIME_CONDITIONS are caps below these):

  name             e     keypoints    what is subnormal (nonzero, below 2^-126) or zero
  natural          0     1155 / 1206  nothing
  small_normal    -40    1155 / 1206  nothing; Ldet peaks at 5e-27 / 1e-26
  ldet_subnormal  -60    1103 / 1157  Ldet 97 % subnormal, 3 % zero (100 % subnormal on its best level); every response subnormal
  ldet_underflow  -64     287 / 332   Ldet 35 % / 37 % subnormal, 65 % / 63 % zero
  deriv_subnormal -120      0         Lx 96 % / 92 %, Lxx 100 %, Lstep 100 % subnormal; Ldet all zero
  lt_subnormal    -127      0         Lt, Lsmooth, every derivative and Lstep 100 % subnormal; Ldet all zero
  last_bits       -145      0         Lt <= 2.4e-44 (17 steps of 2^-149), Lx 93 % / 94 % zero, Lstep 84 % / 80 % zero, Lxx all zero
  large           +20       0         nothing; Ldet peaks at 6.6e9 / 1.4e10 (the sub-pixel step's absolute term rejects all)
  largest_finite  +62       0         nothing; all finite, Ldet peaks at 1.3e35 / 2.7e35, the contrast factor is 1.8e16
"""
import functools

import numpy as np

TINY = np.float32(2.0 ** -126)  # the smallest normal f32
PLANES = ["Lt", "Lsmooth", "Lx", "Ly", "Lxx", "Lyy", "Lxy", "Lflow", "Lstep", "Ldet"]

FRAME_SHAPES = [(320, 160, 11), (327, 163, 12)]  # (w, h, synth_frame index)
FRAME_IDS = [f"{w}x{h}" for w, h, _ in FRAME_SHAPES]

REGIMES = {
    "natural": 0,
    "small_normal": -40,
    "ldet_subnormal": -60,
    "ldet_underflow": -64,
    "deriv_subnormal": -120,
    "lt_subnormal": -127,
    "last_bits": -145,
    "large": 20,
    "largest_finite": 62,
}


def subnormal_share(a):
    """share of the values of `a` that are nonzero and below the smallest normal f32"""
    a = np.abs(np.asarray(a, np.float32))
    return float(((a > 0) & (a < TINY)).mean()) if a.size else 0.0


def zero_share(a):
    a = np.asarray(a, np.float32)
    return float((a == 0).mean()) if a.size else 0.0


def unit(u8):
    """create_unit_float_image (image.rs:136)"""
    return (u8.astype(np.float32) * np.float32(1.0)) / np.float32(255.0)


def frame(amd, w, h, idx, e, signed=False):
    f = unit(amd.synth_frame(w, h, idx))
    if signed:
        f = f - np.float32(0.5)
    return np.ldexp(f, e).astype(np.float32)  # (exact down to e = -118; below that the frame itself loses low bits)


def regime_frame(amd, shape, regime, signed=False):
    w, h, idx = shape
    return frame(amd, w, h, idx, REGIMES[regime], signed)


@functools.lru_cache(maxsize=6)
def oracle_result(ref, amd, shape, regime, signed=False, threshold=0.0):
    """the oracle's extraction of a regime's frame; shared, read-only (a few stay alive, the oldest is dropped)"""
    return ref.extract(regime_frame(amd, shape, regime, signed), ref.default_config(detector_threshold=threshold))


def all_levels(rf, name):
    first = 1 if name in ("Lflow", "Lstep") else 0  # level 0 has neither
    return [rf.plane(l, name) for l in range(first, rf.num_levels)]


def _cat(rf, name):
    return np.concatenate([p.ravel() for p in all_levels(rf, name)])


def _ldet_subnormal(rf):
    return max(subnormal_share(p) for p in all_levels(rf, "Ldet")) > 0.5 and rf.num_keypoints >= 10


def _ldet_underflow(rf):
    d = _cat(rf, "Ldet")
    return zero_share(d) >= 0.10 and subnormal_share(d) >= 0.10 and rf.num_keypoints >= 1


def _deriv_subnormal(rf):
    return subnormal_share(_cat(rf, "Lx")) > 0.5 and subnormal_share(_cat(rf, "Lstep")) > 0.5


def _lt_subnormal(rf):
    lt = np.abs(_cat(rf, "Lt"))
    return bool((lt[lt > 0] < TINY).all()) and bool((lt > 0).any())


def _largest_finite(rf):
    return all(np.isfinite(_cat(rf, n)).all() for n in PLANES) and float(np.abs(_cat(rf, "Ldet")).max()) > 1e30


REGIME_CONDITIONS = {
    "ldet_subnormal": _ldet_subnormal,
    "ldet_underflow": _ldet_underflow,
    "deriv_subnormal": _deriv_subnormal,
    "lt_subnormal": _lt_subnormal,
    "largest_finite": _largest_finite,
}

# by how many binades a plane moves when the frame is multiplied by 2^e: Lflow not at all, Ldet (a product of two second
# derivatives) by 2e, every other plane and the contrast factor by e
PLANE_EXPONENT = {n: 1 for n in PLANES}
PLANE_EXPONENT.update(Lflow=0, Ldet=2)

# ---- per-op inputs -------------------------------------------------------------------------------------------------------
OP_SHAPES = [(37, 53), (64, 64), (33, 130)]
STRIP_SHAPE = (70, 517)  # crosses a 480-column strip of the marches and the streaming kernels
FED_SHAPES = [(3, 3), (64, 5), (33, 130)]
COMMON_EXPS = (0, -100, -120, -126, -140, 60, "bits")
FED_TAUS = np.array([0.19623365730888334, 3.7012260958150769, 0.12604081556156974, 0.25, 1.5, 0.07, 2.2, 0.4,
                     0.9, 0.11, 3.1, 0.6, 0.33])


def eid(e):
    return e if isinstance(e, str) else f"e{e:+d}"


def op_plane(shape, seed, e):
    """uniform(-1, 1) * 2^e as f32; e == "bits": only +-2^-149 and +-0, the last bit of the format"""
    rng = np.random.default_rng(seed)
    if e == "bits":
        last = np.float32(2.0 ** -149)
        return rng.choice(np.array([last, -last, 0.0, -0.0], np.float32), shape)
    return np.ldexp(rng.uniform(-1.0, 1.0, shape), e).astype(np.float32)


# The exponents at which an op's OUTPUT crosses the subnormal boundary on these inputs, part subnormal and part normal (or
# part zero): the oracle's output there is more than 25 % nonzero subnormal, asserted by both test modules on the oracle's
# output alone.  Measured shares, the least over the four shapes:
#   filter (9 random taps) -125: 0.30, -127: 0.91      gaussian_blur -124: 0.75 (sigma 1.0) .. 0.97 (2.5)
#   half_size -124: 0.60                               scharr -123: 0.32 (sigma 1) .. 0.99 (sigma 6)
#   detector_response, Ldet (inputs at 2^e, Ldet at 2^2e) -60: 0.37, -62: 1.00
#   pm_g2 / flow with unit-range gradients and k = 0.0123 * 2^-63: 1.00 / 0.99 (k at 2^-70: 0.13 / 0.59, the rest zero)
#   fed_steps, Lt after the 13 steps, least over FED_SHAPES: -126: 0.32 (flow in (0, 1]) / 1.00 (tiny flow), -128: 0.64 / 1.00
CROSSING = {"filter": (-125, -127), "gaussian_blur": (-124,), "half_size": (-124,), "scharr": (-123,),
            "detector_response": (-60, -62), "pm_g2_k": (-63,), "fed_steps": (-126, -128)}
PM_G2_K_EXTRA = (-70,)  # output part subnormal, mostly zero: not asserted


def detector_expected(ref, ls, sigma):
    lx = ref.scharr(ls, True, False, sigma)
    ly = ref.scharr(ls, False, True, sigma)
    exp = {"Lx": lx, "Ly": ly, "Lxx": ref.scharr(lx, True, False, sigma), "Lyy": ref.scharr(ly, False, True, sigma),
           "Lxy": ref.scharr(lx, False, True, sigma)}
    with np.errstate(under="ignore", over="ignore"):
        exp["Ldet"] = ((exp["Lxx"] * exp["Lyy"]) - (exp["Lxy"] * exp["Lxy"])) * np.float32(sigma ** 4)
    return exp


def fed_expected(ref, lt, flow, taus):
    exp, step = lt.copy(), None
    for t in taus:
        exp, step = ref.fed_step(exp, flow, t)
    return exp, step


def fed_flow(shape, seed, tiny):
    """a conductivity plane in (0, 1], or one that is itself tiny: rand * 2^-130"""
    f = 1.0 - np.random.default_rng(seed).uniform(0.0, 1.0, shape)
    return np.ldexp(f, -130 if tiny else 0).astype(np.float32)


def contrast_images(ref, shape, exps, seed=8):
    """blurred noise at the given exponents, one image per exponent"""
    return np.stack([ref.gaussian_blur(np.ldexp(np.random.default_rng(seed + i).uniform(0.0, 1.0, shape), e).astype(np.float32), 1.6)
                     for i, e in enumerate(exps)])


# The squared gradient magnitude of blurred unit noise is about 2^-8; as an f32 it would turn subnormal near e = -59 and
# vanish near e = -71 (the reference squares in f64, where it never underflows): exponents on both sides of both, and a
# batch of three whose maxima lie tens of orders of magnitude apart
CONTRAST_EXPS = (0, -56, -62, -68, -74, -80, -120, -140, 60)
CONTRAST_BATCHES = ((0, -62, 60), (-140, -74, 0), (-68, 60, -120))
