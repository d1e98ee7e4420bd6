"""The host JPEG decoder (akz_image.cpp: idct, reconstruct_host) against the float64 statement of tests/jpeg_numpy.py, on
streams whose every coefficient is known because the tests wrote them: the IEEE 1180 limits on the transform, its shortcut
paths, its 64-bit range, and the upsampler and colour conversion over twelve sampling-factor sets, four of them with a factor
that does not divide the maximum.  No GPU: tests/test_gpu_jpeg_statement.py holds the kernels to the same statement."""
import os
import sys

import numpy as np
import pytest

import jpeg_numpy as J

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_jpegs  # noqa: E402

SIZES = [(1, 1), (2, 2), (3, 5), (17, 9), (41, 13), (48, 32)]
SETS = {J.factors_id(f): f for f in J.FACTOR_SETS}
ACCURACY = [(lo, hi, sign) for lo, hi in J.ACCURACY_RANGES for sign in (1, -1)]


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("jpeg_statement")


@pytest.fixture(scope="module")
def exact_streams():
    """every exact-tier stream, made once: the colour test and the teeth test share them"""
    return {(n, w, h): J.colour_stream("exact", f, w, h, 100 + k) for n, f in SETS.items() for k, (w, h) in enumerate(SIZES)}


@pytest.mark.parametrize("lo,hi,sign", ACCURACY, ids=[f"{lo}..{hi}x{s}" for lo, hi, s in ACCURACY])
def test_idct_accuracy(amd, folder, lo, hi, sign):
    """IEEE 1180 style: 10 000 blocks, q = 1, coefficients the rounded forward DCT of random samples; the standard's limits
    against ref and an error below 1 against the unrounded value (clipped, where sign -1 takes a sample to 256).  Measured
    on the host decoder, worst of the six streams: peak 1, per-position mean square 0.0211, overall 0.0162, per-position
    mean 0.0041, overall 0.00017; against the unrounded value 0.637."""
    c = J.accuracy_coefs(lo, hi, sign, 10000, 1180 + lo * sign)
    s = J.gray_stream(800, 800, c.reshape(100, 100, 64), [1] * 64)
    got = amd.load_image_luma(s.write(folder, f"acc_{-lo}_{hi}_{sign}.jpg"))
    J.assert_accuracy(J.accuracy_figures(got, s), f"host {lo}..{hi} x{sign}")


def test_basis_and_shortcut_blocks(amd, folder):
    """each coefficient alone at +-A, the column pass's DC shortcut in every column, in none but column 0, in all but one, and
    the all-zero block: within 1 of ref"""
    s = J.strip(J.shortcut_blocks(), [1] * 64)
    got = amd.load_image_luma(s.write(folder, "shortcut.jpg")).astype(np.int64)
    err = np.abs(got - s.ref[0])
    assert err.max() <= 1, (int(err.max()), np.argwhere(err > 1)[0] // 8)
    assert np.array_equal(got[:, -8:], np.full((8, 8), 128))


LARGE = [("8bit_sparse", J.Q8, 2047, 0), ("8bit_dense", J.Q8, 2047, 1), ("16bit_sparse", J.Q16, 32767, 0),
         ("16bit_dense", J.Q16, 32767, 1)]


@pytest.mark.parametrize("name,q,top,dense", LARGE, ids=[m[0] for m in LARGE])
def test_large_magnitudes(amd, folder, name, q, top, dense):
    """|got - clip(exact)| <= 0.5 + 2^-13 * sum |coef * q| over the block, 3 600 blocks per mix.  The 2^-13 covers the 12-bit
    constants of the integer transform.  Measured on the host decoder, the smallest eps that holds (jpeg_numpy.measured_eps):
    3.46e-5 (8-bit sparse), 1.43e-5 (8-bit dense), 2.43e-5 (16-bit sparse), 1.09e-5 (16-bit dense); 2^-13 = 1.22e-4 is three
    and a half times the largest.  Half the blocks carry full-size coefficients and saturate nearly everywhere, so the check
    there is the side of the saturation; the rest are scaled down per block so that samples stay inside 0..255 as well."""
    n = 3600
    s = J.strip(J.large_coefs(top, n, 7 + top + dense, [dense] * n), q)
    got = amd.load_image_luma(s.write(folder, f"large_{name}.jpg"))
    inside = int(((got > 0) & (got < 255)).sum())
    print(f"{name}: measured eps {J.measured_eps(got, s):.3g}, {inside} of {got.size} samples inside 1..254")
    assert inside >= 10  # (not a wholly saturated frame, even at 16-bit tables)
    J.assert_margin(got, s, name)
    x = s.exact[0]
    assert (x < -1e4).any() and (x > 1e4).any()  # (both saturations are in the stream)


def test_extreme_fixture(amd):
    """extreme.jpg (4:2:0, 16-bit tables, coefficients near +-32767, DC up to 32752) through the same margin: the plane
    intervals it gives, propagated through the upsampler, the colour equations and luma"""
    s = J.Stream.of(*make_jpegs.extreme_coefs())
    path = os.path.join(make_jpegs.OUT, "extreme.jpg")
    assert s.data == open(path, "rb").read()
    lo, hi = J.assert_inside(s.margin_bounds(J.EPS), s, amd.load_image_rgb(path), amd.load_image_luma(path), "extreme.jpg")
    assert (lo == hi).mean() > 0.5  # (most of it is pinned: saturated one way or the other)


@pytest.mark.parametrize("name", SETS)
def test_colour_exact(amd, folder, exact_streams, name):
    """DC-only blocks at q[0] = 8: the planes are the integers dc + 128, neighbouring chroma blocks up to 220 levels apart.
    Every stream here agrees on every value, no tie excused."""
    for w, h in SIZES:
        s = exact_streams[name, w, h]
        path = s.write(folder, f"exact_{name}_{w}x{h}.jpg")
        J.assert_exact(s, amd.load_image_rgb(path), amd.load_image_luma(path), (name, w, h))


@pytest.mark.parametrize("name", SETS)
def test_colour_textured(amd, folder, name):
    """six AC coefficients per block in +-40 at q = 3 on top: the planes are ref +- 1, RGB and luma inside the interval"""
    for k, (w, h) in enumerate(SIZES):
        s = J.colour_stream("textured", SETS[name], w, h, 200 + k)
        path = s.write(folder, f"textured_{name}_{w}x{h}.jpg")
        px = amd.load_image_rgb(path)
        J.assert_inside(J.within_one(s.ref), s, px, amd.load_image_luma(path), (name, w, h))
        centre, _ = J.frame_rgb(s.ref, w, h, s.factors)
        print(f"{name} {w}x{h}: at most {np.abs(px.astype(np.int64) - centre).max()} from the centre")


@pytest.mark.parametrize("name", make_jpegs.ENCODED)
def test_encoder_written_fixtures(amd, name):
    """the files of tests/golden/jpeg that the baseline encoder wrote regenerate byte for byte, and (extreme.jpg: above)
    decode inside the textured tier's interval of their coefficients"""
    s = J.Stream.of(*make_jpegs.ENCODED[name]())
    path = os.path.join(make_jpegs.OUT, name)
    assert s.data == open(path, "rb").read(), name
    if name != "extreme.jpg":
        J.assert_inside(J.within_one(s.ref), s, amd.load_image_rgb(path), amd.load_image_luma(path), name)


def test_exact_planes_are_exact(exact_streams):
    """the premise of the exact tier: the f64 planes are the integers dc + 128 of their block"""
    for s in exact_streams.values():
        for x, c in zip(s.exact, s.coefs):
            want = np.repeat(np.repeat(c[..., 0], 8, axis=0), 8, axis=1) + 128
            assert np.abs(x - want).max() < 1e-9


# which exact-tier factor sets must catch each deliberate mistake of the statement's upsampler
CATCHES = {
    "h2v1_round_1": ["2x1-1x1-1x1", "4x2-2x2-1x1", "2x2-2x1-1x2"],
    "far_row_other_side": ["2x2-1x1-1x1", "1x1-2x2-2x2"],
    "neighbour_i_plus_1": ["2x1-1x1-1x1", "2x2-1x1-1x1", "4x2-2x2-1x1", "1x1-2x2-2x2", "2x2-2x1-1x2"],
    "copy_fractional": ["3x1-2x1-1x1", "1x3-1x2-1x1", "4x1-3x1-1x1"],
}


def test_teeth(exact_streams):
    """Every deliberate mistake changes the expected RGB of an exact-tier stream of each factor set CATCHES names for it, and
    of no set without the branch it touches.  Statement against statement: the code under test has no say."""
    assert set(CATCHES) == set(J.MISTAKES)
    right = {k: J.frame_rgb(s.ref, s.w, s.h, s.factors)[0] for k, s in exact_streams.items()}
    for m in J.MISTAKES:
        caught = set()
        for k, s in exact_streams.items():
            if not np.array_equal(J.frame_rgb(s.ref, s.w, s.h, s.factors, (m,))[0], right[k]):
                caught.add(k[0])
        print(f"{m:20s} caught by {sorted(caught)}")
        assert caught == set(CATCHES[m]), (m, sorted(caught))
