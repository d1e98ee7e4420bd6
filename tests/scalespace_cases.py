"""The committed inputs of the scale-space statement (tests/scalespace_numpy.py), shared by tests/test_scalespace_host.py
and tests/test_gpu_scalespace.py.  TEST INFRASTRUCTURE ONLY.  Everything is generated from seeds; there are no fixture files.

The shapes are the smallest at which the front half can still go wrong: 11 x 11 (the smallest accepted frame: the detector's
Scharr of sigma 4 needs 2 * 4 + 3), two strips, 159 x 79 / 160 x 80 (either side of the second octave's admission,
evolution.rs:138-149), 163 x 81 and 130 x 66 (odd sizes; 130 * 66 = 2 mod 4: no plane is a whole number of 4-float vectors),
322 x 200 (three octaves, one pixel row and column above 320 x 160).  Then what a natural frame never shows: constant blocks
with half of them black (exact zero fluxes and planes: compared as WORDS, as is the case with a contrast factor of 0), a flat frame (contrast factor 0, NaN planes:
NaN positions compared), uniform noise, f32 frames scaled down until Ldet underflows (2^-64) and until the derivatives are
subnormal and Ldet is all zero (2^-120, the regimes of tests/range_cases.py), and the Configs that reach other kernel branches.

A case is (name, frame, Config overrides, how its planes are compared: "value" | "words" | "nan").
"""
import functools
import types

import numpy as np

from range_cases import REGIMES, unit

DEFAULTS = dict(num_sublevels=4, max_octave_evolution=4, base_scale_offset=1.6, initial_contrast=0.001, contrast_percentile=0.7,
                contrast_factor_num_bins=300, derivative_factor=1.5, detector_threshold=0.001, descriptor_channels=3,
                descriptor_pattern_size=10)

# base_scale_offset * derivative_factor = 2.5 exactly: level 0's detector sigma lies ON a half (detector_response.rs:24 rounds
# it away from zero, to 3; banker's rounding gives 2).  tests/test_scalespace_host.py checks that it does lie there.
HALF_SIGMA = dict(base_scale_offset=2.5, derivative_factor=1.0)

CONFIGS = {
    "sub3": dict(num_sublevels=3),
    "base2.5": dict(base_scale_offset=2.5),          # a 7-tap level-0 blur, detector sigma 4, 5 and 6
    "deriv2.3": dict(derivative_factor=2.3),         # detector sigma 4, 5 and 6 on the 5-tap blur
    "base1.3": dict(base_scale_offset=1.3),          # ceil(1.3) = 2 but round(1.3) = 1: the kernel size rule shows
    "bins1": dict(contrast_factor_num_bins=1),
    "bins641": dict(contrast_factor_num_bins=641),   # past the 640 bins of the march / stream contrast kernels
    "pct1": dict(contrast_percentile=1.0),
    "pct0": dict(contrast_percentile=0.0),           # the threshold is 0, the factor 0: Lflow is 0 or NaN, fluxes are signed zeros
    "half_sigma": HALF_SIGMA,
}


def config(**kw):
    """anything with Config's attributes"""
    assert not set(kw) - set(DEFAULTS), kw
    return types.SimpleNamespace(**dict(DEFAULTS, **kw))


def natural(w, h, seed):
    """a u8 frame with edges, corners, gradients and texture at several scales: smooth waves, random rectangles, some noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w))
    for _ in range(4):
        fx, fy, ph = rng.uniform(0.02, 0.3), rng.uniform(0.02, 0.3), rng.uniform(0, 6.28)
        img += rng.uniform(10, 30) * np.sin(fx * x + fy * y + ph)
    for _ in range(max(6, w * h // 600)):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        ww, hh = int(rng.integers(2, max(3, w // 4))), int(rng.integers(2, max(3, h // 4)))
        img[y0:y0 + hh, x0:x0 + ww] += rng.uniform(-90, 90)
    img += rng.normal(0, 3, (h, w))
    return np.clip(img + 128, 0, 255).astype(np.uint8)


def blocky(w, h, block, seed):
    """constant blocks, half of them black, as tests/test_gpu_extract.py::test_diffusion_planes_bit_for_bit_on_blocky_frames
    builds them"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, ((h + block - 1) // block, (w + block - 1) // block), dtype=np.uint8)
    coarse[rng.random(coarse.shape) < 0.5] = 0
    return np.ascontiguousarray(np.kron(coarse, np.ones((block, block), np.uint8))[:h, :w])


def scaled(w, h, seed, regime):
    """the f32 unit frame times 2^e, e of the named regime of tests/range_cases.py"""
    return np.ldexp(unit(natural(w, h, seed)), REGIMES[regime]).astype(np.float32)


SIZES = [(11, 11), (12, 40), (2000, 24), (159, 79), (160, 80), (163, 81), (130, 66), (322, 200)]
CONFIG_SIZE = (163, 81)


@functools.lru_cache(maxsize=None)
def cases():
    out = [(f"{w}x{h}", natural(w, h, 100 + i), {}, "value") for i, (w, h) in enumerate(SIZES)]
    out.append(("blocky", blocky(163, 81, 8, 7), {}, "words"))
    out.append(("flat", np.full((61, 97), 77, np.uint8), {}, "nan"))
    out.append(("noise", np.random.default_rng(3).integers(0, 256, (66, 130), dtype=np.uint8), {}, "value"))
    out.append(("ldet_underflow", scaled(160, 80, 200, "ldet_underflow"), {}, "value"))
    out.append(("deriv_subnormal", scaled(163, 81, 201, "deriv_subnormal"), {}, "value"))
    for i, (name, kw) in enumerate(CONFIGS.items()):
        out.append((name, natural(*CONFIG_SIZE, 300 + i), kw, "words" if name == "pct0" else "value"))
    return tuple(out)


CASE_NAMES = [c[0] for c in cases()]


def case(name):
    return cases()[CASE_NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def stated(name, mut=()):
    """the statement's (levels, contrast factor) of a case, computed once, shared and read-only"""
    import scalespace_numpy as S
    _, frame, kw, _ = case(name)
    return S.pyramid(frame, config(**kw), mut)


def planes_equal(a, b, how):
    """two planes of one case: by value (-0.0 == +0.0), NaN positions equal; "words": the words of everything that is no NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na = np.isnan(a)
    if not np.array_equal(na, np.isnan(b)):
        return False
    if how == "words":
        return np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~na])
    return np.array_equal(a[~na], b[~na])


def contrast_equal(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))
