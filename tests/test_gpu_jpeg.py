"""JPEG reconstruction on the device (akz_image_load_luma_device, akz_extract_features_file / _files): the bytes of the host
decoder (akz_image_load_luma) for every fixture, for entropy-coded mutants the host accepts, and the host's errors for
those it refuses; file batches against the oracle and against extract_features on the host-decoded frames."""
import ctypes as C
import glob
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
JPEGS = sorted(glob.glob(os.path.join(GOLDEN, "*.jpg")) + glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg")))
IMG0, IMG1 = os.path.join(GOLDEN, "1.jpg"), os.path.join(GOLDEN, "2.jpg")
POISON = 0xA5


def raw_load(amd, ctx, path, dst, capacity=None):
    """akz_image_load_luma_device through the ABI: (status, message, w, h)."""
    w, h = C.c_uint32(), C.c_uint32()
    ptr = C.c_void_p(dst.data_ptr()) if dst is not None else None
    cap = dst.numel() if capacity is None else capacity
    st = amd.lib().akz_image_load_luma_device(ctx._h, os.fsencode(path), ptr, cap, C.byref(w), C.byref(h))
    msg = amd.lib().akz_last_error().decode() if st else ""
    return st, msg, w.value, h.value


def host_load(amd, path):
    """akz_image_load_luma: (status, message, luma or None)."""
    try:
        return 0, "", amd.load_image_luma(path)
    except amd.AkazeError as e:
        return e.status, amd.lib().akz_last_error().decode(), None


def poison(n):
    import torch
    return torch.full((n,), POISON, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("path", JPEGS, ids=[os.path.relpath(p, GOLDEN) for p in JPEGS])
def test_device_luma_equals_host(ctx, amd, path):
    host = amd.load_image_luma(path)
    dev = ctx.load_luma_device(path)
    assert tuple(dev.shape) == host.shape
    got = dev.cpu().numpy()
    if not np.array_equal(got, host):
        bad = np.argwhere(got != host)
        raise AssertionError(f"{len(bad)} px differ, first {bad[0]}: {got[tuple(bad[0])]} vs {host[tuple(bad[0])]}")


def test_extreme_coefficients(ctx, amd):
    """Dequantised values near +-2^31 (16-bit tables, int16 coefficients): a 32-bit IDCT overflows here."""
    path = os.path.join(GOLDEN, "jpeg", "extreme.jpg")
    host = amd.load_image_luma(path)
    assert len(np.unique(host)) > 2  # (not a saturated frame: the overflow would show)
    assert np.array_equal(ctx.load_luma_device(path).cpu().numpy(), host)


def entropy_segments(data):
    """(start, end) of the entropy-coded data behind every SOS."""
    out, p = [], 2
    while p + 4 <= len(data):
        if data[p] != 0xFF or data[p + 1] in (0x00, 0xFF) or 0xD0 <= data[p + 1] <= 0xD7:
            p += 1
            continue
        m = data[p + 1]
        if m == 0xD9:
            break
        ln = (data[p + 2] << 8) | data[p + 3]
        p += 2 + ln
        if m == 0xDA:
            q = p
            while q + 1 < len(data) and not (data[q] == 0xFF and data[q + 1] not in (0x00,) and not 0xD0 <= data[q + 1] <= 0xD7):
                q += 1
            out.append((p, q))
            p = q
    return out


def test_entropy_mutants(ctx, amd, tmp_path):
    rng = np.random.default_rng(1234)
    accepted = refused = 0
    for name in ("jpeg/s420_257x189.jpg", "jpeg/rst422_65x33.jpg", "jpeg/prog420_97x71.jpg", "jpeg/s411_53x19.jpg",
                 "jpeg/gray_131x67.jpg"):
        data = open(os.path.join(GOLDEN, name), "rb").read()
        segs = entropy_segments(data)
        assert segs, name
        h0, w0 = amd.load_image_luma(os.path.join(GOLDEN, name)).shape
        for k in range(40):
            mut = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                a, b = segs[int(rng.integers(len(segs)))]
                if b > a:
                    mut[int(rng.integers(a, b))] = int(rng.integers(256))
            path = str(tmp_path / f"m{k}.jpg")
            with open(path, "wb") as f:
                f.write(bytes(mut))
            hst, hmsg, host = host_load(amd, path)
            dst = poison(w0 * h0 + 64)
            st, msg, w, h = raw_load(amd, ctx, path, dst)
            assert st == hst, (name, k, st, hst, msg, hmsg)
            if hst:
                refused += 1
                assert msg == hmsg, (name, k)
                assert bool((dst == POISON).all()), (name, k)
            else:
                accepted += 1
                assert (h, w) == host.shape
                got = dst[: w * h].cpu().numpy().reshape(h, w)
                assert np.array_equal(got, host), (name, k)
                assert bool((dst[w * h:] == POISON).all())
    assert accepted >= 50, (accepted, refused)


def test_capacity_and_arguments(ctx, amd):
    path = os.path.join(GOLDEN, "jpeg", "s420_17x9.jpg")
    dst = poison(17 * 9)
    st, _, w, h = raw_load(amd, ctx, path, dst, capacity=17 * 9 - 1)
    assert (st, w, h) == (amd.AKZ_ERR_BUFFER, 17, 9)
    assert bool((dst == POISON).all())
    st, _, w, h = raw_load(amd, ctx, path, None, capacity=0)
    assert (st, w, h) == (amd.AKZ_ERR_BUFFER, 17, 9)
    L = amd.lib()
    wv, hv = C.c_uint32(), C.c_uint32()
    p = C.c_void_p(dst.data_ptr())
    assert L.akz_image_load_luma_device(None, os.fsencode(path), p, 17 * 9, C.byref(wv), C.byref(hv)) == -1
    assert L.akz_image_load_luma_device(ctx._h, None, p, 17 * 9, C.byref(wv), C.byref(hv)) == -1
    assert L.akz_image_load_luma_device(ctx._h, os.fsencode(path), p, 17 * 9, None, C.byref(hv)) == -1
    assert L.akz_image_load_luma_device(ctx._h, os.fsencode(path), None, 17 * 9, C.byref(wv), C.byref(hv)) == -1
    assert bool((dst == POISON).all())
    st, msg, _, _ = raw_load(amd, ctx, os.path.join(GOLDEN, "no_such_file.jpg"), dst)
    assert st == -8 and "cannot read" in msg


def test_png_and_pgm_through_the_device_call(ctx, amd, tmp_path):
    rgb = amd.load_image_rgb(os.path.join(GOLDEN, "jpeg", "s420_257x189.jpg"))
    png = str(tmp_path / "x.png")
    amd.save_png(png, rgb)
    assert np.array_equal(ctx.load_luma_device(png).cpu().numpy(), amd.load_image_luma(png))
    px = np.random.default_rng(5).integers(0, 256, (9, 17), dtype=np.uint8)
    pgm = str(tmp_path / "x.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n# comment\n17 9\n255\n" + px.tobytes())
    assert np.array_equal(amd.load_image_luma(pgm), px)
    assert np.array_equal(ctx.load_luma_device(pgm).cpu().numpy(), px)


def same_result(a, ia, b, ib, planes=()):
    """Image ia of result a equals image ib of result b: keypoints, descriptors, contrast and the named planes."""
    assert a.counts(ia) == b.counts(ib)
    assert a.keypoints(ia).tobytes() == b.keypoints(ib).tobytes()
    assert np.array_equal(a.descriptors(ia), b.descriptors(ib))
    assert a.contrast(ia) == b.contrast(ib)
    for lvl in range(a.counts(ia)[0] if planes else 0):
        for pl in planes:
            assert np.array_equal(a.plane(lvl, pl, ia), b.plane(lvl, pl, ib)), (lvl, pl)


def test_file_batch_matches_oracle_and_frames(ctx, amd, ref):
    import torch
    paths = [IMG0, IMG1, IMG0]
    lumas = [amd.load_image_luma(p) for p in paths]
    frames = torch.from_numpy(np.stack(lumas)).cuda()
    want = ctx.extract_features(frames, keep_all_planes=True)
    ctx.set_host_threads(1)
    try:
        one = ctx.extract_features_files(paths, keep_all_planes=True)
        ctx.set_host_threads(16)
        many = ctx.extract_features_files(paths, keep_all_planes=True)
    finally:
        ctx.set_host_threads(0)
    for i in range(3):
        same_result(one, i, want, i, planes=amd.PLANES if i == 1 else ())
        same_result(many, i, one, i)
    for i in (0, 1):
        q = ref.extract(lumas[i], threads=8)
        nl, nk, nb = many.counts(i)
        assert nk == q.num_keypoints > 100
        assert many.keypoints(i).tobytes() == q.keypoints().tobytes()
        assert np.array_equal(many.descriptors(i), q.descriptors())
        assert many.contrast(i) == q.contrast
        if i == 0:
            for lvl in range(nl):
                for pl in amd.PLANES:
                    a, b = many.plane(lvl, pl, 0), q.plane(lvl, pl)
                    assert a.shape == b.shape and np.array_equal(a, b), (lvl, pl)
    for r in (want, one, many):
        r.close()


def test_file_batch_mixed_formats_and_errors(ctx, amd, tmp_path):
    luma = amd.load_image_luma(IMG1)
    png = str(tmp_path / "2.png")
    amd.save_png(png, luma)
    got = ctx.extract_features_files([IMG0, png], keep_all_planes=False)
    import torch
    want = ctx.extract_features(torch.from_numpy(np.stack([amd.load_image_luma(IMG0), luma])).cuda(), keep_all_planes=False)
    for i in range(2):
        same_result(got, i, want, i)
    small = os.path.join(GOLDEN, "jpeg", "s420_257x189.jpg")
    with pytest.raises(amd.AkazeError) as e:
        ctx.extract_features_files([IMG0, IMG1, small, IMG0])
    assert e.value.status == -1 and "s420_257x189.jpg" in str(e.value)
    with pytest.raises(amd.AkazeError) as e:
        ctx.extract_features_files([IMG0, str(tmp_path / "missing.jpg"), IMG1])
    assert e.value.status == -8 and "missing.jpg" in str(e.value)
    # the context still works after the refused batches
    again = ctx.extract_features_files([IMG0, png], keep_all_planes=False)
    same_result(again, 1, want, 1)


def test_kernel_rows_show_which_path_ran(ctx, amd, tmp_path):
    png = str(tmp_path / "1.png")
    amd.save_png(png, amd.load_image_luma(IMG0))
    ctx.set_profiling(1)
    try:
        ctx.kernel_rows(reset=True)
        r = ctx.extract_features_file(IMG0, keep_all_planes=False)
        rows = ctx.kernel_rows(reset=True)
        kinds = {x["kind"] for x in rows if x["launches"]}
        assert {6, 7, 8} <= kinds, rows
        assert all(x["ms"] > 0 for x in rows if x["kind"] in (6, 7) and x["launches"])
        r.close()
        r = ctx.extract_features_file(png, keep_all_planes=False)
        rows = ctx.kernel_rows(reset=True)
        assert not {x["kind"] for x in rows if x["launches"]} & {6, 7, 8}, rows
        r.close()
    finally:
        ctx.set_profiling(0)


def test_two_contexts_on_two_threads(amd):
    files = [os.path.join(GOLDEN, "jpeg", n) for n in ("s420_257x189.jpg", "s411_53x19.jpg", "prog420_97x71.jpg", "extreme.jpg",
                                                     "rst420_120x88.jpg", "gray_131x67.jpg")]
    host = {p: amd.load_image_luma(p) for p in files}
    errors = []

    def worker(k):
        try:
            c = amd.Context(0)
            try:
                for rnd in range(6):
                    p = files[(rnd * 2 + k) % len(files)]
                    if not np.array_equal(c.load_luma_device(p).cpu().numpy(), host[p]):
                        errors.append((k, rnd, p))
            finally:
                c.close()
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append((k, repr(e)))

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
