"""The detection mask on the GPU: k_mask_candidates alone against the numpy rule (tests/mask_numpy.py), masked extraction against
the statement on the unmasked result's own Ldet planes, the all-ones mask against the unmasked call on every selection path and
call form, the overflow redo, the capacity bookkeeping, the kernel rows, the refusals and the resources.  Bit for bit throughout."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import extrema_numpy as E
import mask_numpy as M
from test_gpu_frames import same_results

pytestmark = pytest.mark.gpu
W, H = 320, 240
INDICES = (100, 126, 143)  # synth_frame indices (chosen with the CPU oracle) at which every partial mask keeps >= 8 and drops >= 8 keypoints
FIELDS = ("x", "y", "response", "size", "octave", "class_id")
POISON = 0xA5
INVALID = -1
SORT_KINDS = (9, 10, 11)  # AKZ_KR_SORT_*


def fresh_context(amd):
    import torch
    return amd.Context(0, torch.cuda.current_stream().cuda_stream)


def keys(kps):
    return set(zip(kps["x"].view(np.uint32).tolist(), kps["y"].view(np.uint32).tolist(), kps["class_id"].tolist()))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(a, pad=13, tail=29, batch=True):
    """a CUDA view of a ([n, h, w] or [h, w] uint8) with a row pitch of w + pad and `tail` bytes between frames, in a poisoned buffer"""
    import torch
    a = np.asarray(a)
    n, (h, w) = (a.shape[0] if a.ndim == 3 else 1), a.shape[-2:]
    stride = h * (w + pad) + tail
    host = np.full(n * stride + 16, POISON, np.uint8)
    for i in range(n):
        rows = host[i * stride:i * stride + h * (w + pad)].reshape(h, w + pad)
        rows[:, :w] = a[i] if a.ndim == 3 else a
    buf = torch.from_numpy(host).cuda()
    if a.ndim == 3 and batch:
        return buf.as_strided((n, h, w), (stride, w + pad, 1))
    return buf.as_strided((h, w), (w + pad, 1))


def levels_of(res):
    infos = [res.level_info(l) for l in range(res.counts(0)[0])]
    return [(i["w"], i["h"], i["octave"], i["esigma"]) for i in infos]


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------

def crafted_list(amd, levels, count, n_img, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros(count, amd.CANDIDATE_IMG_DTYPE)
    rec["level"] = np.arange(count) % len(levels) if count >= len(levels) else rng.integers(0, len(levels), count)
    rec["img"] = rng.integers(0, n_img, count)
    px = np.array([lv[0] * lv[1] for lv in levels])[rec["level"]]
    rec["idx"] = (rng.random(count) * px).astype(np.uint32)
    # the last pixel of some level, and pixel 0: the corners of the mapping
    if count >= 2:
        rec["idx"][0], rec["idx"][1] = px[0] - 1, 0
    for f in ("v", "xp", "xm", "yp", "ym"):
        rec[f] = rng.random(count).astype(np.float32)
    return rec


def run_kernel(amd, ctx, rec, count_word, capacity, mask_t, w, h, n_img, extra=4):
    import torch
    src = np.zeros(capacity, amd.CANDIDATE_IMG_DTYPE)
    src[:min(len(rec), capacity)] = rec[:capacity]
    d_src = dev(src.view(np.uint8))
    d_kept = torch.full(((capacity + extra) * 32,), POISON, dtype=torch.uint8, device="cuda")
    d_cnt = dev(np.array([count_word, 0xDEAD, 0xDEAD, 0xDEAD], np.uint32).view(np.int32))
    ctx.debug_mask_candidates(d_src, capacity, d_cnt, mask_t, w, h, n_img, d_kept)
    ctx.synchronize()
    return d_cnt.cpu().numpy().view(np.uint32), d_kept.cpu().numpy().reshape(capacity + extra, 32)


@pytest.mark.parametrize("shared", [False, True], ids=["per_image", "shared"])
@pytest.mark.parametrize("w,h", [(160, 80), (161, 81)])
def test_kernel_alone(ctx, amd, w, h, shared):
    levels = E.plan_levels(w, h)
    assert [(p["w"], p["h"], p["octave"]) for p in amd.plan_levels(w, h, amd.Config())] == [lv[:3] for lv in levels]
    assert len(levels) == 8 and levels[-1][2] == 1  # two octaves
    rng = np.random.default_rng(w)
    masks = (rng.random((3, h, w)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (3, h, w), dtype=np.uint8)
    masks = masks[0] if shared else masks
    mask_t = pitched(masks)
    assert not mask_t.is_contiguous()
    for count in (0, 1, 63, 64, 65, 4097):
        rec = crafted_list(amd, levels, count, 3, 1000 + count)
        want = rec[M.keep_records(rec, levels, masks)]
        capacity = max(count, 1) + 3
        cnt, kept = run_kernel(amd, ctx, rec, count, capacity, mask_t, w, h, 3)
        assert cnt.tolist() == [len(want), count, 0, 0], (count, cnt)
        got = kept[:len(want)]
        assert sorted(map(bytes, got)) == sorted(r.tobytes() for r in want), count
        assert (kept[len(want):] == POISON).all(), count  # nothing behind the kept records, nothing past the capacity
        if count >= 63:
            assert 0 < len(want) < count


def test_kernel_overflow_leaves_the_count(ctx, amd):
    w, h = 161, 81
    levels = E.plan_levels(w, h)
    masks = np.zeros((h, w), np.uint8)  # (would drop everything)
    rec = crafted_list(amd, levels, 65, 1, 5)
    cnt, kept = run_kernel(amd, ctx, rec, 65, 40, dev(masks), w, h, 1)
    assert cnt.tolist() == [65, 65, 0, 0]
    assert kept[:40].tobytes() == rec[:40].tobytes()  # the truncated list, as the consumers would find it without a mask
    assert (kept[40:] == POISON).all()
    # a count of exactly the capacity is no overflow
    cnt, kept = run_kernel(amd, ctx, rec, 65, 65, dev(masks + 1), w, h, 1)
    assert cnt.tolist() == [65, 65, 0, 0] and sorted(map(bytes, kept[:65])) == sorted(r.tobytes() for r in rec)
    assert (kept[65:] == POISON).all()


# ---- masked extraction equals the statement -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scenes(amd, ctx):
    """the frames on the device in two producers' forms, and each form's unmasked result (n = 3), computed once"""
    grey = np.stack([amd.synth_frame(W, H, k) for k in INDICES])
    forms = {"rgb": (dev(np.stack([grey] * 3, axis=-1)), "hwc"), "grey_pitched": (pitched(grey, pad=7, tail=0), "hw")}
    out = {}
    for name, (t, layout) in forms.items():
        res = ctx.extract_frames(t, layout)
        out[name] = dict(t=t, layout=layout, res=res, levels=levels_of(res),
                         ldets=[[res.plane(l, "Ldet", i) for l in range(res.counts(i)[0])] for i in range(3)])
    yield out
    for v in out.values():
        v["res"].close()


_stated = {}


def stated(scene_name, scene, img, mask_name):
    """detect_masked on the unmasked result's Ldet planes, then that result's own orientation and descriptors: computed once"""
    key = (scene_name, img, mask_name)
    if key not in _stated:
        kps, _ = M.detect_masked(scene["ldets"][img], scene["levels"], E_CFG(), M.make_mask(mask_name, W, H))
        if len(kps):
            kps, desc = scene["res"].describe_keypoints(kps, img=img, compute_orientation=True)
        else:
            desc = np.zeros((0, 61), np.uint8)
        _stated[key] = (kps, desc)
    return _stated[key]


@functools.lru_cache(maxsize=None)
def E_CFG():
    """the default Config: the statement reads its derivative_factor and detector_threshold"""
    import akaze_amd
    return akaze_amd.Config()


def check_against_statement(scene_name, scene, got, imgs, mask_names):
    unmasked = scene["res"]
    for k, (img, mask_name) in enumerate(zip(imgs, mask_names)):
        want, desc = stated(scene_name, scene, img, mask_name)
        kp = got.keypoints(k)
        assert len(kp) == len(want), (scene_name, img, mask_name, len(kp), len(want))
        for f in FIELDS + ("angle",):
            a, b = np.asarray(kp[f]), np.asarray(want[f])
            if a.dtype.kind == "f":
                a, b = a.view(np.uint32), b.view(np.uint32)
            assert np.array_equal(a, b), (scene_name, img, mask_name, f)
        assert np.array_equal(got.descriptors(k), desc), (scene_name, img, mask_name)
        # the pyramid is untouched by the mask
        assert got.contrast(k) == unmasked.contrast(img)
        last = got.counts(k)[0] - 1
        for plane in ("Lt", "Ldet"):
            assert got.plane(last, plane, k).tobytes() == unmasked.plane(last, plane, img).tobytes(), (mask_name, plane)
        # the condition on the inputs: a partial mask keeps and drops at least 8 keypoints of this frame
        full = unmasked.keypoints(img)
        if mask_name in M.PARTIAL:
            assert len(want) >= 8 and len(keys(full) - keys(want)) >= 8, (scene_name, img, mask_name, len(want), len(full))
        elif mask_name == "ones":
            assert kp.tobytes() == full.tobytes() and len(full) >= 8
        else:
            assert len(kp) == 0


@pytest.mark.parametrize("mask_name", ["ones", "zeros"] + list(M.PARTIAL))
def test_shared_mask_rgb_batch(ctx, amd, scenes, mask_name):
    sc = scenes["rgb"]
    mask = dev(M.make_mask(mask_name, W, H)) if mask_name != "rows2" else dev(M.make_mask(mask_name, W, H) != 0)  # (a torch bool tensor too)
    got = ctx.extract_frames(sc["t"], sc["layout"], mask=mask)
    check_against_statement("rgb", sc, got, (0, 1, 2), [mask_name] * 3)
    got.close()


def test_per_frame_masks_pitched_grey_batch(ctx, amd, scenes):
    sc = scenes["grey_pitched"]
    for names in (("checker8", "rows2", "left_half"), ("disc", "ones", "zeros")):
        masks = pitched(np.stack([M.make_mask(m, W, H) for m in names]))
        got = ctx.extract_frames(sc["t"], sc["layout"], mask=masks)
        check_against_statement("grey_pitched", sc, got, (0, 1, 2), names)
        got.close()


@pytest.mark.parametrize("scene_name", ["rgb", "grey_pitched"])
def test_single_frame(ctx, amd, scenes, scene_name):
    """n = 1: a shared [H, W] mask and a per-frame [1, H, W] mask, on a view of the batch's first frame"""
    sc = scenes[scene_name]
    m = M.make_mask("checker8", W, H)
    for mask in (pitched(m), dev(m[None])):
        got = ctx.extract_frames(sc["t"][:1], sc["layout"], mask=mask)
        check_against_statement(scene_name, sc, got, (0,), ("checker8",))
        got.close()


# ---- all ones equals unmasked: every selection path, every call form ------------------------------------------------------------

@pytest.fixture(scope="module")
def three(amd, ctx, scenes):
    """three one-frame RGB jobs, a mask for each (all ones, checkerboard, every second row) and each one's synchronous results"""
    ts = [scenes["rgb"]["t"][k:k + 1] for k in range(3)]
    masks = [dev(M.make_mask(m, W, H)) for m in ("ones", "checker8", "rows2")]
    plain = [ctx.extract_frames(t) for t in ts]
    masked = [ctx.extract_frames(t, mask=m) for t, m in zip(ts, masks)]
    same_results(masked[0], plain[0], 1)
    for k, name in enumerate(("ones", "checker8", "rows2")):  # what the call forms below are compared with is the statement's
        check_against_statement("rgb", scenes["rgb"], masked[k], (k,), (name,))
    yield ts, masks, plain, masked
    for r in plain + masked:
        r.close()


@pytest.mark.parametrize("setter,value", [("debug_set_select", 0), ("debug_set_select", 1), ("debug_set_select", 2), ("debug_set_host_sort", True),
                                          ("debug_set_device_libm", False)])
def test_every_selection_path(ctx, amd, scenes, three, setter, value):
    ts, masks, plain, masked = three
    sc = scenes["rgb"]
    ones = dev(np.ones((H, W), np.uint8))
    getattr(ctx, setter)(value)
    try:
        got = ctx.extract_frames(sc["t"], mask=ones)
        same_results(got, sc["res"], 3)
        got.close()
        for k in range(3):
            got = ctx.extract_frames(ts[k], mask=masks[k])
            same_results(got, masked[k], 1)
            got.close()
    finally:
        getattr(ctx, setter)(None)


@pytest.mark.parametrize("input_ready", [False, True], ids=["on_stream", "input_ready"])
def test_three_jobs_in_flight(ctx, amd, three, input_ready):
    ts, masks, plain, masked = three
    ctx.synchronize()
    for order in ((0, 1, 2), (2, 1, 0)):
        jobs = [ctx.extract_frames_begin(t, input_ready=input_ready, mask=m) for t, m in zip(ts, masks)]
        res = {k: jobs[k].finish() for k in order}
        for k in range(3):
            same_results(res[k], masked[k], 1)
            res[k].close()
    same_results(masked[0], plain[0], 1)


def test_abandon_between_two_finished(ctx, amd, three):
    ts, masks, plain, masked = three
    jobs = [ctx.extract_frames_begin(t, mask=m) for t, m in zip(ts, masks)]
    first = jobs[0].finish()
    jobs[1].abandon()
    last = jobs[2].finish()
    again = ctx.extract_frames_begin(ts[1], mask=masks[1]).finish()
    for r, k in ((first, 0), (last, 2), (again, 1)):
        same_results(r, masked[k], 1)
        r.close()


def test_two_lanes(amd, three):
    ts, masks, plain, masked = three
    c = fresh_context(amd)
    try:
        c.set_lanes(2)
        order = (0, 1, 2, 0)
        jobs = [c.extract_frames_begin(ts[k], input_ready=(i % 2 == 1), mask=masks[k]) for i, k in enumerate(order)]
        res = [j.finish() for j in jobs]
        for r, k in zip(res, order):
            same_results(r, masked[k], 1)
            r.close()
        assert c.debug_mask_counts()["kept"] > 0
    finally:
        c.close()


def test_host_call_equals_device_call(ctx, amd):
    luma = amd.synth_frame(W, H, INDICES[0])
    for name in ("ones", "checker8"):
        m = M.make_mask(name, W, H)
        host = ctx.extract_features_masked(luma, m != 0)
        device = ctx.extract_frames(dev(luma), layout="hw", mask=dev(m))
        same_results(host, device, 1)
        if name == "ones":
            plain = ctx.extract_features(luma)
            same_results(host, plain, 1)
            plain.close()
        host.close()
        device.close()
    _, kp, desc = amd.extract_features(luma, ctx=ctx, mask=M.make_mask("checker8", W, H))
    assert len(kp) >= 8 and desc.shape == (len(kp), 61)


# ---- overflow, bookkeeping, rows, refusals, resources ---------------------------------------------------------------------------

def mask_rows(amd, c):
    return [r for r in c.kernel_rows(reset=True) if r["kind"] == amd.KR_MASK_CANDIDATES]


def test_overflow_redo_goes_through_the_mask(amd, three):
    ts, masks, plain, masked = three
    c = fresh_context(amd)
    try:
        c.set_profiling(1)
        c.set_candidate_hint(16)
        got = c.extract_frames(ts[1], mask=masks[1])
        same_results(got, masked[1], 1)
        got.close()
        counts = c.debug_mask_counts()
        assert counts["redone"] == 1 and 16 < counts["kept"] < counts["unfiltered"], counts
        rows = mask_rows(amd, c)
        assert len(rows) == 1 and rows[0]["launches"] == 2, rows
    finally:
        c.close()


def texture(w, h, seed, block=8):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, ((h + block - 1) // block, (w + block - 1) // block), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((block, block), np.uint8))[:h, :w])


def test_bookkeeping_sees_the_unfiltered_count(amd):
    """A stream of heavily masked frames must not pick the 8 192-entry short list: the next extrema pass appends the UNFILTERED
    list.  1 024 x 768 of random 8-pixel blocks: about 38 000 candidates (CPU oracle), of which a tenth-wide strip keeps 2 100."""
    w, h = 1024, 768
    frame = dev(texture(w, h, 11))
    mask = dev(M.make_mask("tenth", w, h))
    c = fresh_context(amd)
    try:
        c.set_profiling(1)
        plain0 = c.extract_frames(frame, layout="hw", keep_all_planes=False)
        first = None
        for k in range(4):
            got = c.extract_frames(frame, layout="hw", mask=mask, keep_all_planes=False)
            counts = c.debug_mask_counts()
            assert counts["unfiltered"] > 8192 and counts["kept"] * 10 < counts["unfiltered"] and counts["kept"] > 64, counts
            if k >= 1:
                assert counts["redone"] == 0, (k, counts)
                assert got.keypoints(0).tobytes() == first
            else:
                first = got.keypoints(0).tobytes()
            got.close()
        c.kernel_rows(reset=True)
        plain1 = c.extract_frames(frame, layout="hw", keep_all_planes=False)
        sort_rows = [r for r in c.kernel_rows(reset=True) if r["kind"] in SORT_KINDS]
        # (the sort's row carries the list's capacity: with room for the unfiltered list the extrema pass is not redone)
        assert sum(r["launches"] > 0 for r in sort_rows) == 1 and sum(r["px"] for r in sort_rows) >= counts["unfiltered"], sort_rows
        same_results(plain1, plain0, 1, planes=False)
        assert not mask_rows(amd, c)
        plain0.close()
        plain1.close()
    finally:
        c.close()


def test_no_mask_nothing_new(amd, three):
    ts, masks, plain, masked = three
    c = fresh_context(amd)
    try:
        c.set_profiling(1)
        for _ in range(2):
            c.extract_frames(ts[0]).close()
        c.extract_frames_begin(ts[0]).finish().close()
        assert not mask_rows(amd, c)
        gc.collect()
        blocks = amd.debug_resource_counts()["device_blocks"]
        c.extract_frames(ts[0]).close()
        assert amd.debug_resource_counts()["device_blocks"] == blocks
        assert not mask_rows(amd, c)
        c.extract_frames(ts[0], mask=masks[1]).close()
        rows = mask_rows(amd, c)
        assert len(rows) == 1 and (rows[0]["launches"], rows[0]["kernel"], rows[0]["param"], rows[0]["w"], rows[0]["h"], rows[0]["n"]) == \
            (1, "k_mask_candidates", 1, W, H, 1), rows
        assert rows[0]["ms"] > 0
        assert amd.debug_resource_counts()["device_blocks"] > blocks
        jobs = [c.extract_frames_begin(ts[k], mask=masks[k]) for k in range(3)]
        for j in jobs:
            j.finish().close()
        rows = mask_rows(amd, c)
        assert len(rows) == 1 and rows[0]["launches"] == 3, rows
    finally:
        c.close()


def test_refusals_enqueue_nothing(ctx, amd, three):
    ts, masks, plain, masked = three
    t = three[0][0]
    n = 3
    frames = dev(np.zeros((n, H, W), np.uint8))
    mask = dev(np.ones((n, H, W), np.uint8))
    fl = amd.FrameLayout(amd.FRAME_GRAY8, W, H, 0, 0, 0)
    G = amd.FRAME_GRAY8
    trials = [("d_mask", 0, (G, W, H, 0, 0, 0), n), ("mask_layout", mask.data_ptr(), None, n),
              ("format", mask.data_ptr(), (amd.FRAME_RGB8, W, H, 0, 0, 0), n), ("width", mask.data_ptr(), (G, W + 1, H, 0, 0, 0), n),
              ("height", mask.data_ptr(), (G, W, H - 1, 0, 0, 0), n), ("n_masks", mask.data_ptr(), (G, W, H, 0, 0, 0), 2),
              ("n_masks", mask.data_ptr(), (G, W, H, 0, 0, 0), 0), ("row_pitch", mask.data_ptr(), (G, W, H, W - 1, 0, 0), n),
              ("frame_stride", mask.data_ptr(), (G, W, H, 0, W * H - 1, 0), n)]
    cfg = amd.Config()
    L = amd.lib()
    ctx.set_profiling(1)
    try:
        ctx.kernel_rows(reset=True)
        for field, ptr, fields, n_masks in trials:
            ml = amd.FrameLayout(*fields) if fields is not None else None
            for fn in (L.akz_extract_device_frames_masked, L.akz_extract_begin_device_frames_masked):
                out = C.c_void_p(0xDEAD)
                st = fn(ctx._h, C.c_void_p(frames.data_ptr()), C.byref(fl), n, C.c_void_p(ptr) if ptr else None,
                        C.byref(ml) if ml is not None else None, n_masks, C.byref(cfg), 0, C.byref(out))
                msg = L.akz_last_error().decode()
                assert st == INVALID and not out.value and field in msg and fn.__name__ in msg, (field, st, out.value, msg)
        assert not [r for r in ctx.kernel_rows(reset=True) if r["launches"]]
        # both null: the unmasked call
        out = C.c_void_p()
        assert L.akz_extract_device_frames_masked(ctx._h, C.c_void_p(t.data_ptr()), C.byref(amd.FrameLayout(amd.FRAME_RGB8, W, H, 0, 0, 0)), 1,
                                                  None, None, 0, C.byref(cfg), 0, C.byref(out)) == 0
        r = amd.ExtractResult(ctx, out)
        assert r.keypoints(0).tobytes() == plain[0].keypoints(0).tobytes()
        r.close()
        assert not mask_rows(amd, ctx)
    finally:
        ctx.set_profiling(0)
    for bad, word in ((mask.float(), "uint8 or bool"), (mask[:, :, :-1], "the mask is"), (mask[:2], "2 masks for 3"),
                      (dev(np.ones((n, H, 2 * W), np.uint8))[:, :, ::2], "pixel stride")):
        with pytest.raises(ValueError, match=word):
            ctx.extract_frames(frames, layout="hw", mask=bad)
    with pytest.raises(ValueError, match="CUDA"):
        ctx.extract_frames_begin(frames, layout="hw", mask=np.ones((H, W), np.uint8))


def test_resources_and_scratch(amd, three):
    ts, masks, plain, masked = three
    gc.collect()
    before = amd.debug_resource_counts()
    c = fresh_context(amd)
    try:
        c.debug_set_alloc_fill(True)

        def audit(what):
            rows = c.debug_audit_scratch()
            assert not [r for r in rows if r["first_bad"] is not None], (what, rows)

        r = c.extract_frames(ts[1], mask=masks[1], keep_all_planes=False)
        audit("masked")
        assert r.keypoints(0).tobytes() == masked[1].keypoints(0).tobytes()
        r.close()
        r = c.extract_frames(ts[1], keep_all_planes=False)
        audit("unmasked")
        assert r.keypoints(0).tobytes() == plain[1].keypoints(0).tobytes()
        r.close()
        jobs = [c.extract_frames_begin(t, mask=m, keep_all_planes=False) for t, m in zip(ts, masks)]
        jobs[1].abandon()
        for k in (0, 2):
            r = jobs[k].finish()
            assert r.keypoints(0).tobytes() == masked[k].keypoints(0).tobytes()
            r.close()
        audit("jobs")
        luma = amd.synth_frame(W, H, INDICES[0])
        c.extract_features_masked(luma, M.make_mask("disc", W, H), keep_all_planes=False).close()
        assert amd.debug_resource_counts()["device_bytes"] > before["device_bytes"]
    finally:
        c.close()
    gc.collect()
    after = amd.debug_resource_counts()
    assert after == before, {k: after[k] - before[k] for k in before}
