"""akz_luma_from_frames_host -- the host statement of frame ingest (include/akaze_hip.h: akz_frame_layout) -- against a numpy float32
statement of DynamicImage::to_luma written here, bit for bit: every (R, G, B) triple once, the six formats over a matrix of
shapes, pitches, frame and plane strides with poison round every declared row and round the output, the image loaders'
own luma for the colour fixtures, the Python view mapping (crops, non-contiguous batches), and every refusal."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import frames_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("akz_luma_from_frames_host", "akz_luma_from_frames_device", "akz_extract_device_frames", "akz_extract_begin_device_frames")
INVALID = -1
GUARD = 32


def raw_host(amd, src, fields, n, dst):
    """akz_luma_from_frames_host through the ABI: (status, message); src / dst: numpy uint8 or None"""
    lay = amd.FrameLayout(*fields) if fields is not None else None
    st = amd.lib().akz_luma_from_frames_host(C.c_void_p(src.ctypes.data) if src is not None else None, C.byref(lay) if lay is not None else None,
                                             n, C.c_void_p(dst.ctypes.data) if dst is not None else None)
    return st, amd.lib().akz_last_error().decode() if st else ""


def run_case(amd, case):
    """the statement on a case, into a buffer with poison guards in front and behind"""
    px = case.n * case.h * case.w
    out = np.full(px + 2 * GUARD, fc.POISON, np.uint8)
    st, msg = raw_host(amd, case.buf, case.fields, case.n, out[GUARD:])
    assert st == 0, (case, st, msg)
    assert (out[:GUARD] == fc.POISON).all() and (out[GUARD + px:] == fc.POISON).all(), case
    return out[GUARD:GUARD + px].reshape(case.n, case.h, case.w)


def test_symbols_exported_and_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "akaze_hip_debug.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in L._declared, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert "typedef struct akz_frame_layout" in hdr and "typedef enum akz_frame_format" in hdr
    for k, name in enumerate(("GRAY8", "RGB8", "BGR8", "RGBA8", "BGRA8", "RGB8_PLANAR")):
        assert re.search(r"AKZ_FRAME_" + name + r"\s*=\s*%d\b" % k, hdr), name
        assert getattr(amd, "FRAME_" + name) == k
    assert re.search(r"AKZ_KR_FRAME_LUMA\s*=\s*12\b", dbg) and amd.KR_FRAME_LUMA == 12
    assert C.sizeof(amd.FrameLayout) == 40
    assert L.akz_abi_version() == 6
    for name in ("luma_from_frames", "extract_frames", "extract_frames_begin"):
        assert callable(getattr(amd.Context, name)), name
    assert callable(amd.luma_from_frames_host)


def test_grey_sent_as_rgb_is_not_the_identity(amd):
    """(v, v, v) -> v fails first at 13: a grey picture sent as RGB is not its own luma, in numpy and in the library alike"""
    v = np.arange(256, dtype=np.uint8)
    l = fc.luma_numpy(v, v, v)
    assert (l[:13] == v[:13]).all() and l[13] == 12
    assert np.array_equal(amd.luma_from_frames_host(np.stack([v, v, v], axis=-1)[None]), l[None])


def test_every_rgb_triple(amd):
    case = fc.all_triples()
    got = run_case(amd, case)
    want = case.expected()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("fmt", sorted(fc.FORMATS), ids=[fc.FORMATS[f] for f in sorted(fc.FORMATS)])
def test_matrix_equals_numpy(amd, fmt):
    count = 0
    for case in fc.matrix(fmt):
        assert np.array_equal(run_case(amd, case), case.expected()), case
        count += 1
    assert count == 13 * 4 * 2 * 4 * 2 * (2 if fmt == fc.PLANAR else 1)


def colour_fixtures(amd):
    out = []
    for p in [os.path.join(GOLDEN, "1.jpg")] + sorted(glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg"))):
        try:
            if amd.load_image(p).ndim == 3:
                out.append(p)
        except amd.AkazeError:
            pass  # (fixtures the decoder refuses on purpose)
    return out


def test_image_loaders_agree(amd):
    paths = colour_fixtures(amd)
    assert os.path.join(GOLDEN, "1.jpg") in paths and len(paths) >= 4, paths
    for p in paths:
        rgb, luma = amd.load_image_rgb(p), amd.load_image_luma(p)
        assert np.array_equal(amd.luma_from_frames_host(rgb), luma), p


def test_python_views(amd):
    """crops, channel orders, planar and non-contiguous batches map onto the layout with no copy"""
    rng = np.random.default_rng(5)
    parent = rng.integers(0, 256, (4, 30, 40, 4), dtype=np.uint8)
    r, g, b = (parent[..., k] for k in range(3))
    full = fc.luma_numpy(r, g, b)
    assert np.array_equal(amd.luma_from_frames_host(parent), full)
    assert np.array_equal(amd.luma_from_frames_host(parent, order="bgr"), fc.luma_numpy(b, g, r))
    assert np.array_equal(amd.luma_from_frames_host(parent[:, 3:29, 7:, :]), full[:, 3:29, 7:])
    assert np.array_equal(amd.luma_from_frames_host(parent[::2, 5:6, 1:2, :]), full[::2, 5:6, 1:2])
    assert np.array_equal(amd.luma_from_frames_host(parent[1, 2:, :33]), full[1, 2:, :33])
    rgb = np.ascontiguousarray(parent[..., :3])
    assert np.array_equal(amd.luma_from_frames_host(rgb[:, ::2]), full[:, ::2])  # (every second row: a pitch)
    chw = np.ascontiguousarray(rgb.transpose(0, 3, 1, 2))
    assert np.array_equal(amd.luma_from_frames_host(chw, layout="chw"), full)
    assert np.array_equal(amd.luma_from_frames_host(chw[1:, :, 4:, 5:31], layout="chw"), full[1:, 4:, 5:31])
    grey = np.ascontiguousarray(r)
    assert np.array_equal(amd.luma_from_frames_host(grey, layout="hw"), r)
    assert np.array_equal(amd.luma_from_frames_host(grey[:, 2:9, 3:], layout="hw"), r[:, 2:9, 3:])
    for bad, kw, word in ((rgb[:, :, ::2], {}, "pixel stride"), (rgb[:, ::-1], {}, "row stride"), (rgb[::-1], {}, "frame stride"),
                          (rgb.transpose(0, 2, 1, 3), {}, "pixel stride"), (rgb[..., ::-1], {}, "channel stride"),
                          (chw[:, ::-1], dict(layout="chw"), "plane stride"), (chw, dict(layout="chw", order="bgr"), "planar"),
                          (np.broadcast_to(rgb[0, 0], (5, 40, 3)), {}, "row stride"), (rgb[..., :2], {}, "channels"),
                          (rgb.astype(np.float32), {}, "uint8")):
        with pytest.raises(ValueError, match=word):
            amd.luma_from_frames_host(bad, **kw)


def test_refusals_write_nothing(amd):
    case = fc.Case(fc.RGB8, 8, 4, 2, rng=np.random.default_rng(1))
    planar = fc.Case(fc.PLANAR, 8, 4, 2, rng=np.random.default_rng(2))
    f, w, h = case.fields[:3]
    trials = [
        ("src", None, case.fields, 2, True),
        ("layout", case.buf, None, 2, True),
        ("n", case.buf, case.fields, 0, True),
        ("format", case.buf, (6, w, h, 0, 0, 0), 2, True),
        ("format", case.buf, (0xFFFFFFFF, w, h, 0, 0, 0), 2, True),
        ("width", case.buf, (f, 0, h, 0, 0, 0), 2, True),
        ("height", case.buf, (f, w, 0, 0, 0, 0), 2, True),
        ("row_pitch", case.buf, (f, w, h, 3 * w - 1, 0, 0), 2, True),
        ("row_pitch", case.buf, (f, w, h, 1, 0, 0), 2, True),
        ("frame_stride", case.buf, (f, w, h, 0, 3 * w * h - 1, 0), 2, True),
        ("frame_stride", case.buf, (f, w, h, 3 * w + 2, (3 * w + 2) * h - 1, 0), 2, True),
        ("plane_stride", planar.buf, (fc.PLANAR, w, h, 0, 0, w * h - 1), 2, True),
        ("plane_stride", planar.buf, (fc.PLANAR, w, h, w + 3, 0, (w + 3) * h - 1), 2, True),
        ("frame_stride", planar.buf, (fc.PLANAR, w, h, 0, 3 * (w * h + 5) - 1, w * h + 5), 2, True),
        ("luma", case.buf, case.fields, 2, False),
    ]
    for field, src, fields, n, with_dst in trials:
        out = np.full(2 * w * h + 2 * GUARD, fc.POISON, np.uint8)
        st, msg = raw_host(amd, src, fields, n, out[GUARD:] if with_dst else None)
        assert st == INVALID, (field, st)
        assert field in msg and "akz_luma_from_frames_host" in msg, (field, msg)
        assert (out == fc.POISON).all(), field
    # the tight values themselves, spelled out, are accepted
    out = np.empty(2 * w * h, np.uint8)
    assert raw_host(amd, case.buf, (f, w, h, 3 * w, 3 * w * h, 0), 2, out)[0] == 0
    assert np.array_equal(out.reshape(2, h, w), case.expected())
