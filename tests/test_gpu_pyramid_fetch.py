"""akz_fetch_pyramid / ExtractResult.pyramid: a whole EvolutionStep pyramid in one call.  Bar: every plane byte for byte
what plane() (akz_fetch_plane) and the oracle return, whatever the destination memory, subset or in-flight job."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PLANES = ["Lt", "Lsmooth", "Lx", "Ly", "Lxx", "Lyy", "Lxy", "Lflow", "Lstep", "Ldet"]
LEAN_RECOMPUTED = ["Lxx", "Lyy", "Lxy", "Lstep"]
AKZ_ERR_INVALID_ARG = -1
SENTINEL = 0x7FC0DEAD  # a NaN no plane holds


def frame_input(amd, w, h, idx, kind):
    import torch
    f = amd.synth_frame(w, h, idx)
    if kind == "u8":
        return f
    if kind == "f32":
        return f.astype(np.float32) / np.float32(255.0)
    return torch.from_numpy(f).cuda()


def assert_pyramid_is_plane(res, pyr, img=0, planes=PLANES):
    nl = res.counts(img)[0]
    assert len(pyr) == nl
    for lvl in range(nl):
        assert sorted(pyr[lvl]) == sorted(planes)
        for pl in planes:
            a, b = pyr[lvl][pl], res.plane(lvl, pl, img)
            assert a.shape == b.shape, (lvl, pl, a.shape, b.shape)
            assert a.tobytes() == b.tobytes(), (img, lvl, pl)


def sentinel_bufs(res, img=0):
    """one sentinel-filled buffer per (level, plane), sized as akz_result_level_info says (level 0 Lflow / Lstep: 1 float)"""
    bufs = []
    for lvl in range(res.counts(img)[0]):
        info = res.level_info(lvl)
        for pl in PLANES:
            n = 1 if lvl == 0 and pl in ("Lflow", "Lstep") else info["w"] * info["h"]
            bufs.append(np.full(n, SENTINEL, np.uint32).view(np.float32))
    return bufs


def raw_fetch(amd, res, img, bufs, pass_only=None, n_dst=None):
    """akz_fetch_pyramid on per-plane buffers; entries whose plane is not in pass_only are NULL"""
    ptrs = (C.c_void_p * len(bufs))()
    for i, b in enumerate(bufs):
        if pass_only is None or PLANES[i % 10] in pass_only:
            ptrs[i] = b.ctypes.data
    n = C.c_uint64(12345)
    rc = amd.lib().akz_fetch_pyramid(res._h, img, ptrs, len(bufs) if n_dst is None else n_dst, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("kind", ["u8", "f32", "device"])
@pytest.mark.parametrize("keep", [True, False], ids=["all", "lean"])
@pytest.mark.parametrize("cfg", ["default", "5x5ch1"])
@pytest.mark.parametrize("w,h", [(11, 11), (97, 61), (640, 480), (1920, 1080)])
def test_pyramid_matches_plane(ctx, amd, w, h, cfg, keep, kind):
    options = amd.Config() if cfg == "default" else amd.Config(num_sublevels=5, max_octave_evolution=5,
                                                               descriptor_channels=1)
    res = ctx.extract_features(frame_input(amd, w, h, 11, kind), options, keep_all_planes=keep)
    pyr = res.pyramid()
    assert_pyramid_is_plane(res, pyr)
    assert pyr[0]["Lflow"].shape == (0, 0) and pyr[0]["Lstep"].shape == (0, 0)


@pytest.mark.parametrize("keep", [True, False], ids=["all", "lean"])
def test_pyramid_batch_stride(ctx, amd, keep):
    import torch
    frames = np.stack([amd.synth_frame(163, 81, i) for i in range(3)])
    res = ctx.extract_features(torch.from_numpy(frames).cuda(), keep_all_planes=keep)
    pyrs = [res.pyramid(img=i) for i in range(3)]
    for i in range(3):
        assert_pyramid_is_plane(res, pyrs[i], img=i)
    for pl in PLANES:  # the images differ, so a wrong stride could not go unnoticed
        for lvl in (0, 4):
            if pyrs[0][lvl][pl].size:
                assert pyrs[0][lvl][pl].tobytes() != pyrs[1][lvl][pl].tobytes() != pyrs[2][lvl][pl].tobytes(), (lvl, pl)


@pytest.mark.parametrize("w,h,keep", [(1920, 1080, True), (640, 480, False)])
def test_pyramid_matches_oracle(ctx, amd, ref, w, h, keep):
    frame = amd.synth_frame(w, h, 21)
    res = ctx.extract_features(frame, keep_all_planes=keep)
    rf = ref.extract(frame, threads=8)
    pyr = res.pyramid()
    assert len(pyr) == rf.num_levels
    for lvl in range(rf.num_levels):
        for pl in PLANES:
            b = rf.plane(lvl, pl)
            assert pyr[lvl][pl].shape == b.shape, (lvl, pl)
            assert pyr[lvl][pl].tobytes() == b.tobytes(), (lvl, pl)
    rf.close()


@pytest.mark.parametrize("subset,keep", [(("Lt", "Ldet"), True), (("Lt", "Ldet"), False), (LEAN_RECOMPUTED, False)],
                         ids=["Lt+Ldet-all", "Lt+Ldet-lean", "recomputed-lean"])
def test_pyramid_subsets_leave_the_rest_untouched(ctx, amd, subset, keep):
    res = ctx.extract_features(amd.synth_frame(321, 243, 5), keep_all_planes=keep)
    bufs = sentinel_bufs(res)
    rc, nbytes = raw_fetch(amd, res, 0, bufs, pass_only=subset)
    assert rc == 0
    want = 0
    for i, b in enumerate(bufs):
        lvl, pl = divmod(i, 10)
        pl = PLANES[pl]
        if pl in subset and not (lvl == 0 and pl in ("Lflow", "Lstep")):
            ref_plane = res.plane(lvl, pl).reshape(-1)
            assert b.tobytes() == ref_plane.tobytes(), (lvl, pl)
            want += b.nbytes
        else:
            assert (b.view(np.uint32) == SENTINEL).all(), (lvl, pl)
    assert nbytes == want
    # the binding's subset form returns those planes only, with the same bytes
    assert_pyramid_is_plane(res, res.pyramid(planes=list(subset)), planes=list(subset))


@pytest.mark.parametrize("w,h,keep", [(1920, 1080, True), (640, 480, False)])
def test_pyramid_destination_kinds(ctx, amd, w, h, keep):
    import torch
    res = ctx.extract_features(amd.synth_frame(w, h, 8), keep_all_planes=keep)
    n = res.pyramid_floats()
    pinned = torch.empty(n, dtype=torch.float32, pin_memory=True).numpy()
    raw = np.empty(n * 4 + 128, np.uint8)
    off = (4 - raw.ctypes.data) % 64  # 4-byte but not 64-byte aligned
    odd = raw[off:off + n * 4].view(np.float32)
    assert odd.ctypes.data % 64 == 4
    a = res.pyramid()
    b = res.pyramid(out=pinned)
    c = res.pyramid(out=odd)
    assert b[0]["Lt"].ctypes.data == pinned.ctypes.data and c[0]["Lt"].ctypes.data == odd.ctypes.data
    assert pinned.tobytes() == odd.tobytes()
    assert_pyramid_is_plane(res, a)
    for lvl in range(len(a)):
        for pl in PLANES:
            assert a[lvl][pl].tobytes() == b[lvl][pl].tobytes() == c[lvl][pl].tobytes(), (lvl, pl)


def test_pyramid_repeatable_on_a_lean_result(ctx, amd):
    res = ctx.extract_features(amd.synth_frame(640, 480, 9), keep_all_planes=False)
    first = res.pyramid()
    second = res.pyramid()
    for lvl in range(len(first)):
        for pl in PLANES:
            assert first[lvl][pl].tobytes() == second[lvl][pl].tobytes(), (lvl, pl)


@pytest.mark.parametrize("eager", [True, False], ids=["eager-finish", "caller-finish"])
def test_pyramid_fetch_during_another_job(amd, ref, eager):
    """Job B begun on the same context, A's pyramid fetched, then B finished: both still equal the oracle."""
    import torch
    ctx = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        ctx.set_eager_finish(eager)
        fa, fb = amd.synth_frame(640, 480, 31), amd.synth_frame(640, 480, 32)
        res_a = ctx.extract_features(fa, keep_all_planes=False)
        db = torch.from_numpy(fb).cuda().unsqueeze(0)
        job = ctx.extract_begin(db, keep_all_planes=False)
        pyr = res_a.pyramid()
        res_b = job.finish()
        ra, rb = ref.extract(fa), ref.extract(fb)
        for lvl in range(ra.num_levels):
            for pl in PLANES:
                assert pyr[lvl][pl].tobytes() == ra.plane(lvl, pl).tobytes(), (lvl, pl)
        kb, rkb = res_b.keypoints(), rb.keypoints()
        assert len(kb) == len(rkb) > 0
        for f in ("x", "y", "response", "size", "octave", "class_id", "angle"):
            assert kb[f].tobytes() == rkb[f].tobytes(), f
        assert res_b.descriptors().tobytes() == rb.descriptors().tobytes()
        ra.close()
        rb.close()
        res_a.close()
        res_b.close()
    finally:
        ctx.close()


def test_pyramid_argument_errors_write_nothing(ctx, amd):
    res = ctx.extract_features(amd.synth_frame(97, 61, 2), keep_all_planes=False)
    nl = res.counts(0)[0]
    bufs = sentinel_bufs(res)
    untouched = lambda: all((b.view(np.uint32) == SENTINEL).all() for b in bufs)
    rc, n = raw_fetch(amd, res, 1, bufs)  # img out of range (one image)
    assert rc == AKZ_ERR_INVALID_ARG and n == 12345 and untouched()
    rc, n = raw_fetch(amd, res, 0, bufs, n_dst=nl * 10 - 1)
    assert rc == AKZ_ERR_INVALID_ARG and n == 12345 and untouched()
    n = C.c_uint64(12345)
    assert amd.lib().akz_fetch_pyramid(res._h, 0, None, nl * 10, C.byref(n)) == AKZ_ERR_INVALID_ARG
    assert n.value == 12345 and untouched()
    assert b"akz_fetch_pyramid" in amd.lib().akz_last_error()
    # and a valid call on the same buffers still works afterwards
    rc, n = raw_fetch(amd, res, 0, bufs)
    assert rc == 0 and n > 0 and not untouched()
