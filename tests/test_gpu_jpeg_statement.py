"""k_jpeg_idct and k_jpeg_luma (csrc/akz_jpeg.hip) against the float64 statement of tests/jpeg_numpy.py, on streams whose
every coefficient is known because the tests wrote them.  For every stream the device frame equals the host decoder's bit
for bit (as tests/test_gpu_jpeg.py asks of the fixtures) and satisfies the statement directly: the IEEE 1180 limits and
the large-magnitude margin on gray, equality with the luma of the statement's RGB where the planes are exact, the luma
interval where they carry the transform's +-1.  Shapes sit on the kernels' boundaries: 8 blocks per wave and 32 per
workgroup in k_jpeg_idct, components that change inside a wave, 256 pixels per workgroup in k_jpeg_luma."""
import os
import sys

import numpy as np
import pytest

import jpeg_numpy as J

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_jpegs  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (2, 2), (3, 5), (17, 9), (255, 3), (256, 4), (257, 5)]
SETS = {J.factors_id(f): f for f in J.FACTOR_SETS}
STRIPS = [1, 7, 8, 9, 31, 32, 33, 65]
GRAY_SIZES = [(1, 1), (7, 9), (255, 3)]


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("jpeg_statement_gpu")


@pytest.fixture(scope="module")
def load(ctx, amd, folder):
    """writes a stream and returns the device's frame, after holding it to the host decoder's bit for bit"""
    def run(s, name):
        return both(ctx, amd, s.write(folder, name + ".jpg"), name)
    return run


def both(ctx, amd, path, what):
    host = amd.load_image_luma(path)
    dev = ctx.load_luma_device(path).cpu().numpy()
    assert dev.shape == host.shape, what
    bad = np.argwhere(dev != host)
    assert not len(bad), (what, len(bad), bad[0], dev[tuple(bad[0])], host[tuple(bad[0])])
    return dev


def assert_peak(got, s, what):
    """a gray frame within 1 of ref and less than 1 from the unrounded value (the per-sample limits of IEEE 1180; its means
    need the 10 000 blocks of test_idct_accuracy)"""
    e = np.abs(got.astype(np.int64) - s.ref[0][:s.h, :s.w])
    u = np.abs(got - np.clip(s.exact[0][:s.h, :s.w], 0, 255))
    assert e.max() <= J.PEAK and u.max() < 1, (what, int(e.max()), float(u.max()))


@pytest.mark.parametrize("n", STRIPS)
def test_gray_strips(load, n):
    """one block high, n blocks: the last wave and the last workgroup of k_jpeg_idct partly filled, and just full"""
    s = J.strip(J.accuracy_coefs(-128, 127, 1, n, n), [1] * 64)
    assert_peak(load(s, f"strip{n}"), s, n)


@pytest.mark.parametrize("w,h", GRAY_SIZES)
def test_gray_sizes(load, w, h):
    """gray frames that end inside their last blocks: k_jpeg_luma crops the plane"""
    bw, bh = -(-w // 8), -(-h // 8)
    s = J.gray_stream(w, h, J.accuracy_coefs(-128, 127, -1, bw * bh, w).reshape(bh, bw, 64), [1] * 64)
    assert_peak(load(s, f"gray{w}x{h}"), s, (w, h))


def test_basis_and_shortcut_blocks(load):
    s = J.strip(J.shortcut_blocks(), [1] * 64)
    got = load(s, "shortcut")
    assert_peak(got, s, "shortcut")
    assert np.array_equal(got[:, -8:], np.full((8, 8), 128))


@pytest.mark.parametrize("name,q,top", [("8bit", J.Q8, 2047), ("16bit", J.Q16, 32767)])
def test_large_magnitudes(load, name, q, top):
    """256 blocks, sparse and dense in turn, at the margin tests/test_jpeg_statement_host.py measures and asserts"""
    n = 256
    s = J.strip(J.large_coefs(top, n, 11 + top, [(b // 2) % 2 for b in range(n)]), q)
    got = load(s, "large_" + name)
    print(f"{name}: measured eps {J.measured_eps(got, s):.3g}")
    J.assert_margin(got, s, name)
    assert len(np.unique(got)) > 2


def test_idct_accuracy(load):
    """the IEEE 1180 limits over 10 000 blocks (313 workgroups of k_jpeg_idct); the figures are the host decoder's, whose
    bytes these are: tests/test_jpeg_statement_host.py"""
    s = J.gray_stream(800, 800, J.accuracy_coefs(-128, 127, 1, 10000, 1180 - 128).reshape(100, 100, 64), [1] * 64)
    J.assert_accuracy(J.accuracy_figures(load(s, "accuracy"), s), "device -128..127")


@pytest.mark.parametrize("tier", ["exact", "textured"])
@pytest.mark.parametrize("w,h,factors", [(16, 16, J.FACTOR_SETS[2]), (24, 8, J.FACTOR_SETS[8])], ids=["4+1+1", "3+2+1"])
def test_components_inside_one_wave(load, tier, w, h, factors):
    """six blocks in all: the three components share one wave of k_jpeg_idct, which picks table and plane by blk0"""
    s = J.colour_stream(tier, factors, w, h, 31)
    assert sum(c.shape[0] * c.shape[1] for c in s.coefs) == 6
    got = load(s, f"wave_{tier}_{w}x{h}")
    if tier == "exact":
        J.assert_exact(s, None, got, (w, h))
    else:
        J.assert_inside(J.within_one(s.ref), s, None, got, (w, h))


@pytest.mark.parametrize("name", SETS)
def test_colour_exact(load, name):
    """every factor set at widths around the 256 pixels of a k_jpeg_luma workgroup and at sizes inside one MCU; planes exact"""
    for k, (w, h) in enumerate(SIZES):
        s = J.colour_stream("exact", SETS[name], w, h, 300 + k)
        J.assert_exact(s, None, load(s, f"exact_{name}_{w}x{h}"), (name, w, h))


@pytest.mark.parametrize("name", SETS)
def test_colour_textured(load, name):
    for k, (w, h) in enumerate(SIZES):
        s = J.colour_stream("textured", SETS[name], w, h, 400 + k)
        J.assert_inside(J.within_one(s.ref), s, None, load(s, f"textured_{name}_{w}x{h}"), (name, w, h))


@pytest.mark.parametrize("name", make_jpegs.ENCODED)
def test_encoder_written_fixtures(ctx, amd, name):
    """the fixtures the baseline encoder wrote, from the coefficients their generators give: inside the textured tier's
    interval; extreme.jpg inside the interval its large-magnitude margin gives"""
    s = J.Stream.of(*make_jpegs.ENCODED[name]())
    path = os.path.join(make_jpegs.OUT, name)
    assert s.data == open(path, "rb").read(), name
    bounds = s.margin_bounds(J.EPS) if name == "extreme.jpg" else J.within_one(s.ref)
    J.assert_inside(bounds, s, None, both(ctx, amd, path, name), name)
