"""Frame ingest on the device (akz_luma_from_frames_device, akz_extract_device_frames, akz_extract_begin_device_frames): k_frame_luma
against the host statement bit for bit -- the matrix of test_frames_host.py, misaligned bases, offsets beyond 2^32 -- and
extraction from colour, cropped and pitched frames against extract_features on the host statement's luma: synchronous,
begun and finished in any order, run ahead, abandoned, on lanes, and against the file path."""
import ctypes as C
import os

import numpy as np
import pytest

import frames_cases as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG0 = os.path.join(ROOT, "tests", "golden", "1.jpg")
W, H = 320, 240
GUARD = 8
INVALID = -1


def fresh_context(amd):
    import torch
    return amd.Context(0, torch.cuda.current_stream().cuda_stream)


def raw_device(amd, ctx, src_ptr, fields, n, dst_ptr):
    lay = amd.FrameLayout(*fields) if fields is not None else None
    st = amd.lib().akz_luma_from_frames_device(ctx._h, C.c_void_p(src_ptr) if src_ptr else None, C.byref(lay) if lay is not None else None, n,
                                               C.c_void_p(dst_ptr) if dst_ptr else None)
    return st, amd.lib().akz_last_error().decode() if st else ""


def run_cases(amd, ctx, cases, src_shift=lambda k: k % 4, dst_shift=lambda k: 0):
    """every case through k_frame_luma: the sources in one upload (case k at a 16-byte boundary + src_shift(k)), the outputs in one
    poisoned buffer with GUARD bytes between them (+ dst_shift(k)), one download; each output and its guards are checked"""
    import torch
    src_off, dst_off, s, d = [], [], 0, GUARD
    for k, c in enumerate(cases):
        s = (s + 15) // 16 * 16 + src_shift(k)
        src_off.append(s)
        s += len(c.buf)
        d += dst_shift(k)
        dst_off.append(d)
        d += c.n * c.h * c.w + GUARD
    host = np.full(s + 16, fc.POISON, np.uint8)
    for c, o in zip(cases, src_off):
        host[o:o + len(c.buf)] = c.buf
    src = torch.from_numpy(host).cuda()
    dst = torch.full((d + 16,), fc.POISON, dtype=torch.uint8, device="cuda")
    for c, so, do in zip(cases, src_off, dst_off):
        st, msg = raw_device(amd, ctx, src.data_ptr() + so, c.fields, c.n, dst.data_ptr() + do)
        assert st == 0, (c, st, msg)
    ctx.synchronize()
    out = dst.cpu().numpy()
    covered = np.zeros(len(out), bool)
    for c, do in zip(cases, dst_off):
        px = c.n * c.h * c.w
        got = out[do:do + px].reshape(c.n, c.h, c.w)
        assert np.array_equal(got, c.expected()), (c, np.argwhere(got != c.expected())[:4])
        covered[do:do + px] = True
    assert (out[~covered] == fc.POISON).all(), np.flatnonzero((out != fc.POISON) & ~covered)[:8]


@pytest.mark.parametrize("fmt", sorted(fc.FORMATS), ids=[fc.FORMATS[f] for f in sorted(fc.FORMATS)])
def test_matrix_equals_host_statement(ctx, amd, fmt):
    cases = list(fc.matrix(fmt))
    for c in cases[::97]:  # (the expectation is numpy's; that the host statement says the same is test_frames_host.py's whole matrix)
        out = np.empty(c.n * c.h * c.w, np.uint8)
        lay = amd.FrameLayout(*c.fields)
        assert amd.lib().akz_luma_from_frames_host(C.c_void_p(c.buf.ctypes.data), C.byref(lay), c.n, C.c_void_p(out.ctypes.data)) == 0
        assert np.array_equal(out.reshape(c.n, c.h, c.w), c.expected()), c
    run_cases(amd, ctx, cases)


def test_every_rgb_triple(ctx, amd):
    run_cases(amd, ctx, [fc.all_triples()])


def test_misaligned_bases(ctx, amd):
    """source and destination bases offset by 0 .. 3 bytes, every format, a wide odd row (1021 x 5: several workgroups per row)
    and a narrow one, with pitches that give every row another alignment"""
    rng = np.random.default_rng(77)
    cases, shifts = [], []
    for fmt in sorted(fc.FORMATS):
        for (w, h, n, pe) in ((1021, 5, 2, 1), (65, 3, 1, 0), (1021, 5, 1, 0)):
            for ss in range(4):
                for ds in range(4):
                    cases.append(fc.Case(fmt, w, h, n, pe, 0, 3 if fmt == fc.PLANAR else 0, rng))
                    shifts.append((ss, ds))
    run_cases(amd, ctx, cases, src_shift=lambda k: shifts[k][0], dst_shift=lambda k: shifts[k][1])


def test_offsets_beyond_4gib(ctx, amd):
    """two 64 x 48 RGB frames 2^32 + 64 bytes apart in ONE allocation: a 32-bit offset would read 64 bytes into the first frame"""
    import torch
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    stride = 2 ** 32 + 64
    big = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
    for i in range(2):
        big[i * stride:i * stride + frames[i].size] = torch.from_numpy(frames[i].reshape(-1)).cuda()
    view = big.as_strided((2, 48, 64, 3), (stride, 64 * 3, 3, 1))
    got = ctx.luma_from_frames(view)
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy(), amd.luma_from_frames_host(frames))
    del view, big


# ---- extraction --------------------------------------------------------------------------------------------------------------

def channels(amd, firsts, w=W, h=H):
    """the R, G, B (and a fourth) channel of len(firsts) frames, [n, h, w] each: frame i is made of the four different pictures
    synth_frame(w, h, firsts[i] + 0 .. 3) (indices whose luma has 8 or more keypoints at these sizes, by the CPU oracle)"""
    return [np.stack([amd.synth_frame(w, h, f + k) for f in firsts]) for k in range(4)]


def as_view(kind, ch):
    """(numpy array in the producer's form, layout, order) for channels ch"""
    r, g, b, a = ch
    if kind == "rgb8":
        return np.stack([r, g, b], axis=-1), "hwc", "rgb"
    if kind == "bgra8":
        return np.stack([b, g, r, a], axis=-1), "hwc", "bgr"
    return np.stack([r, g, b], axis=1), "chw", "rgb"


def same_results(a, b, n, planes=True):
    """keypoints (all fields), descriptors, contrast and the last level's Lt / Ldet of every image, bit for bit"""
    for i in range(n):
        ka, kb = a.keypoints(i), b.keypoints(i)
        assert len(ka) == len(kb) and len(ka) > 0, (i, len(ka), len(kb))
        assert ka.tobytes() == kb.tobytes(), i
        assert np.array_equal(a.descriptors(i), b.descriptors(i)), i
        assert a.contrast(i) == b.contrast(i), i
        if planes:
            last = a.counts(i)[0] - 1
            for name in ("Lt", "Ldet"):
                assert a.plane(last, name, i).tobytes() == b.plane(last, name, i).tobytes(), (i, name)


def reference(amd, ctx, arr, layout, order):
    """extract_features on the host statement's luma of the same bytes"""
    import torch
    return ctx.extract_features(torch.from_numpy(amd.luma_from_frames_host(arr, layout, order)).cuda())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", ["rgb8", "bgra8", "planar"])
def test_extract_frames_equals_extract_on_luma(ctx, amd, kind, n):
    import torch
    arr, layout, order = as_view(kind, channels(amd, (40, 44, 32)[:n]))
    got = ctx.extract_frames(torch.from_numpy(arr).cuda(), layout, order)
    want = reference(amd, ctx, arr, layout, order)
    same_results(got, want, n)
    got.close()
    want.close()


def test_extract_crop_view(ctx, amd):
    """a region of a 400 x 300 parent as a strided view: no copy, keypoint coordinates relative to the crop"""
    import torch
    arr, layout, order = as_view("rgb8", channels(amd, (8, 40), 400, 300))
    parent = torch.from_numpy(arr).cuda()
    view, host = parent[:, 30:30 + H, 41:41 + W, :], arr[:, 30:30 + H, 41:41 + W, :]
    assert not view.is_contiguous()
    got = ctx.extract_frames(view)
    want = reference(amd, ctx, host, layout, order)
    same_results(got, want, 2)
    kp = got.keypoints(0)
    assert kp["x"].max() < W and kp["y"].max() < H
    got.close()
    want.close()


def test_extract_gray_with_pitch(ctx, amd):
    import torch
    luma = np.stack([amd.synth_frame(W, H, k) for k in (66, 67)])
    padded = np.full((2, H, W + 7), fc.POISON, np.uint8)
    padded[:, :, :W] = luma
    got = ctx.extract_frames(torch.from_numpy(padded).cuda()[:, :, :W], layout="hw")
    want = ctx.extract_features(torch.from_numpy(luma).cuda())
    same_results(got, want, 2)
    tight = ctx.extract_frames(torch.from_numpy(luma).cuda(), layout="hw")  # (packed luma: handed to the extraction as it is)
    same_results(tight, want, 2, planes=False)
    for r in (got, want, tight):
        r.close()


@pytest.fixture(scope="module")
def three(amd, ctx):
    """three different RGB batches (1 frame each) on the device and each one's synchronous result"""
    import torch
    ts = [torch.from_numpy(as_view("rgb8", channels(amd, (f,)))[0]).cuda() for f in (20, 100, 68)]
    res = [ctx.extract_frames(t) for t in ts]
    yield ts, res
    for r in res:
        r.close()


def batch_path_context(amd):
    c = fresh_context(amd)
    c.debug_set_schedule(4, 1)  # SCHED_JOB_KPX: every job takes the batch path
    c.debug_set_schedule(6, 1)  # SCHED_PREP_OWN_LAUNCH: the automatic preparation, which is what runs ahead
    c.debug_set_schedule(0, 1)  # SCHED_EARLY_STREAM: the copy stream, whatever the placement probe found
    return c


@pytest.mark.parametrize("where", ["context", "batch_path"])
@pytest.mark.parametrize("input_ready", [False, True], ids=["on_stream", "input_ready"])
def test_three_jobs_in_flight(ctx, amd, three, input_ready, where):
    """each job's luma frames live in its own slot's staging buffer: a shared one would give a job another job's picture"""
    ts, sync = three
    c = ctx if where == "context" else batch_path_context(amd)
    try:
        c.synchronize()
        for order in ((0, 1, 2), (2, 1, 0)):
            jobs = [c.extract_frames_begin(t, input_ready=input_ready) for t in ts]
            res = {k: jobs[k].finish() for k in order}
            for k in range(3):
                same_results(res[k], sync[k], 1)
                res[k].close()
    finally:
        if c is not ctx:
            c.close()


def test_abandon_between_two_finished(ctx, amd, three):
    ts, sync = three
    for input_ready in (False, True):
        jobs = [ctx.extract_frames_begin(t, input_ready=input_ready) for t in ts]
        first = jobs[0].finish()
        jobs[1].abandon()
        last = jobs[2].finish()
        same_results(first, sync[0], 1)
        same_results(last, sync[2], 1)
        again = ctx.extract_frames_begin(ts[1]).finish()  # (the abandoned job's slot is free again)
        same_results(again, sync[1], 1, planes=False)
        for r in (first, last, again):
            r.close()


def test_lanes(amd, three):
    """four small jobs dealt to two lanes (conversion behind the lane_in wait, or on the lane's copy stream)"""
    ts, sync = three
    c = fresh_context(amd)
    try:
        c.set_lanes(2)
        order = (0, 1, 2, 0)
        jobs = [c.extract_frames_begin(ts[k], input_ready=(i % 2 == 1)) for i, k in enumerate(order)]
        res = [j.finish() for j in jobs]
        for r, k in zip(res, order):
            same_results(r, sync[k], 1)
            r.close()
    finally:
        c.close()


def test_file_equivalence(ctx, amd):
    """the same picture through the file path and through device frames: 2016 x 1512, three components"""
    import torch
    rgb = amd.load_image_rgb(IMG0)
    assert rgb.shape == (1512, 2016, 3)
    got = ctx.extract_frames(torch.from_numpy(rgb).cuda(), layout="hwc", keep_all_planes=False)
    want = ctx.extract_features_file(IMG0, keep_all_planes=False)
    ka, kb = got.keypoints(0), want.keypoints(0)
    assert len(ka) == len(kb) > 0 and ka.tobytes() == kb.tobytes()
    assert np.array_equal(got.descriptors(0), want.descriptors(0))
    got.close()
    want.close()


def test_refusals_enqueue_nothing(ctx, amd):
    import torch
    case = fc.Case(fc.RGB8, W, H, 1, rng=np.random.default_rng(3))
    src = torch.from_numpy(case.buf).cuda()
    f, w, h = case.fields[:3]
    trials = [("src", 0, case.fields, 1), ("layout", src.data_ptr(), None, 1), ("n", src.data_ptr(), case.fields, 0),
              ("format", src.data_ptr(), (6, w, h, 0, 0, 0), 1), ("width", src.data_ptr(), (f, 0, h, 0, 0, 0), 1),
              ("height", src.data_ptr(), (f, w, 0, 0, 0, 0), 1), ("row_pitch", src.data_ptr(), (f, w, h, 3 * w - 1, 0, 0), 1),
              ("frame_stride", src.data_ptr(), (f, w, h, 0, 3 * w * h - 1, 0), 2),
              ("plane_stride", src.data_ptr(), (fc.PLANAR, w, h, 0, 0, w * h - 1), 1)]
    dst = torch.full((w * h,), fc.POISON, dtype=torch.uint8, device="cuda")
    cfg = amd.Config()
    L = amd.lib()
    for field, ptr, fields, n in trials:
        lay = amd.FrameLayout(*fields) if fields is not None else None
        layp = C.byref(lay) if lay is not None else None
        st, msg = raw_device(amd, ctx, ptr, fields, n, dst.data_ptr())
        assert st == INVALID and field in msg, (field, st, msg)
        for fn in (L.akz_extract_device_frames, L.akz_extract_begin_device_frames):
            out = C.c_void_p(0xDEAD)
            st = fn(ctx._h, C.c_void_p(ptr) if ptr else None, layp, n, C.byref(cfg), 0, C.byref(out))
            assert st == INVALID and not out.value and field in L.akz_last_error().decode(), (field, st, out.value)
    assert raw_device(amd, ctx, src.data_ptr(), case.fields, 1, 0)[0] == INVALID
    ctx.synchronize()
    assert bool((dst == fc.POISON).all())
    # frames too small for the stencils keep the extraction's own status
    tiny = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(amd.AkazeError) as e_frames:
        ctx.extract_frames(tiny)
    with pytest.raises(amd.AkazeError) as e_luma:
        ctx.extract_features(tiny[..., 0].contiguous())
    assert e_frames.value.status == e_luma.value.status == -4
    with pytest.raises(ValueError, match="channel stride"):
        ctx.extract_frames(src.new_zeros((1, 8, 8, 6))[..., ::2])
    with pytest.raises(ValueError, match="pixel stride"):
        ctx.extract_frames(src.new_zeros((1, 8, 16, 3))[:, :, ::2])


def test_resources_come_back(amd, three):
    """create / frames workload / destroy: the owning types' counters return to their first reading"""
    import gc
    ts, sync = three
    gc.collect()
    before = amd.debug_resource_counts()
    c = fresh_context(amd)
    kps = []
    try:
        r = c.extract_frames(ts[0], keep_all_planes=False)
        kps.append(r.keypoints(0).tobytes())
        r.close()
        for input_ready in (False, True):
            jobs = [c.extract_frames_begin(t, input_ready=input_ready, keep_all_planes=False) for t in ts]
            for j in jobs:
                r = j.finish()
                kps.append(r.keypoints(0).tobytes())
                r.close()
        assert amd.debug_resource_counts()["device_bytes"] > before["device_bytes"]
    finally:
        c.close()
    gc.collect()
    after = amd.debug_resource_counts()
    assert after == before, {k: after[k] - before[k] for k in before}
    assert kps == [sync[k].keypoints(0).tobytes() for k in (0, 0, 1, 2, 0, 1, 2)]


def test_profile_row(ctx, amd):
    import torch
    arr, layout, order = as_view("rgb8", channels(amd, (40, 44)))
    t = torch.from_numpy(arr).cuda()
    ctx.set_profiling(1)
    try:
        ctx.kernel_rows(reset=True)
        r = ctx.extract_frames(t, keep_all_planes=False)
        rows = [x for x in ctx.kernel_rows(reset=True) if x["kind"] == amd.KR_FRAME_LUMA]
        assert len(rows) == 1, rows
        row = rows[0]
        assert (row["launches"], row["px"], row["param"], row["w"], row["h"], row["n"]) == (1, 2 * W * H, amd.FRAME_RGB8, W, H, 2), row
        assert row["ms"] > 0, row
        r.close()
    finally:
        ctx.set_profiling(0)
