"""The feature bank on the GPU (akz_bank_*, k_bank_gather, the bank forms of the seeded pairs calls; include/akaze_hip.h).

The scene: 320 x 240 synthetic frames that are shifted copies of one another, so that pairs really match, and one flat frame,
which gives a set of 0 keypoints.  Two results -- one batched extraction of (frame, flat frame, shifted frame) and one lone
extraction -- give a bank of four sets whose segment table has an empty segment in the middle.  The reference of every equality
is akz_match_features_seeded_pairs / _pose_pairs over the results' host copies, computed once per option set and left unchanged;
everything is compared as bytes.

Model kinds: the library has three, numbered 0 (homography), 1 (fundamental) and 3 (normalised fundamental); all three are
covered, and model_kind 2, which no call accepts, must be refused alike by both forms."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 320, 240
INVALID_ARG = -1
# a repeated pair, a reversed pair, (a, a), a pair whose first set is empty, one whose second set is empty; set 3 is only ever second
PAIRS = [(0, 2), (0, 2), (2, 0), (0, 0), (1, 0), (0, 1), (2, 3), (0, 3)]
EPSILON = {0: 3.0, 1: 0.02, 3: 2.0}  # pixels for a homography, the algebraic residual at unit norm, Sampson pixels
BASE = (1 << 64) - 3              # the pairs' streams wrap around


def frames(amd):
    flat = np.full((H, W), 128, np.uint8)
    return [amd.synth_frame(W, H, 0), flat, amd.synth_frame(W, H, 0, shift=(5, 3))], amd.synth_frame(W, H, 0, shift=(-4, 2))


def extract(amd, ctx, options=None):
    """-> [the batched result of three images, the lone result]"""
    import torch
    three, lone = frames(amd)
    return [ctx.extract_features(torch.from_numpy(np.stack(three)).cuda(), options, keep_all_planes=False),
            ctx.extract_features(torch.from_numpy(lone).cuda(), options, keep_all_planes=False)]


def host_sets(results):
    return [(r.keypoints(i), r.descriptors(i)) for r in results for i in range(r.num_images)]


@pytest.fixture(scope="module")
def scene(amd, ctx):
    """(host sets, bank from the results, bank from the host sets); the results are closed before anything uses the banks"""
    results = extract(amd, ctx)
    feats = host_sets(results)
    padded = [np.pad(d, ((0, 0), (0, 64 - d.shape[1]))) for _, d in feats]
    bank = ctx.feature_bank(results)
    for r in results:
        r.close()
    from_sets = ctx.feature_bank(feats)
    counts = [len(k) for k, _ in feats]
    assert counts[1] == 0 and min(counts[0], counts[2], counts[3]) >= 16, counts
    yield feats, padded, bank, from_sets
    bank.close()
    from_sets.close()


def option_sets(amd, kinds, guided=(0, 1)):
    for kind, cross, its, g, conf in itertools.product(kinds, (False, True), (0, 2), guided, (0.0, 0.99)):
        opt = amd.RansacOptions(model_kind=kind, max_trials=256, confidence=conf, refine_iterations=its, epsilon_inliers=EPSILON[kind],
                                stream_base=BASE, guided=g, guided_radius=3.0, guided_lowes_ratio=0.9)
        yield (kind, cross, its, g, conf), opt, cross


def as_bytes(rows):
    """one call's per-pair tuples -> per pair a tuple of bytes / ints: every output array as words"""
    out = []
    for row in rows:
        cells = []
        for v in row:
            if v is None or isinstance(v, int):
                cells.append(v)
            elif hasattr(v, "words"):
                cells.append(v.words().tobytes())
            else:
                cells.append((v.dtype.str, v.shape, np.ascontiguousarray(v).tobytes()))
        out.append(tuple(cells))
    return out


CAMERAS = [(400.0 + 3 * s, 400.0 - 2 * s, 160.0 + s, 120.0 - s) for s in range(4)]


@pytest.fixture(scope="module")
def expected(amd, ctx, scene):
    """the sets calls over the host copies: {option key: outputs}, for the plain and for the pose call (computed once)"""
    feats = scene[0]
    plain = {key: as_bytes(ctx.match_features_seeded_pairs(feats, PAIRS, opt, cross_check=cross)) for key, opt, cross in option_sets(amd, (0, 1, 3))}
    pose = {key: as_bytes(ctx.match_features_seeded_pose_pairs(feats, CAMERAS, PAIRS, opt, cross_check=cross, points=True))
            for key, opt, cross in option_sets(amd, (1, 3), guided=(0,))}
    # the scene does its job: related pairs find models and keep lists, pairs with an empty set keep nothing
    key = (1, False, 2, 0, 0.99)
    lists = [np.frombuffer(c[0][2], amd.MATCH_DTYPE) for c in plain[key]]
    assert min(len(lists[p]) for p in (0, 1, 2, 6, 7)) >= 8 and len(lists[4]) == 0 and len(lists[5]) == 0, [len(m) for m in lists]
    assert all(plain[key][p][1] is not None for p in (0, 1, 2, 6, 7)) and plain[key][4][1] is None and plain[key][5][1] is None
    assert all(pose[(1, False, 2, 0, 0.99)][p][1] is not None for p in (0, 2, 6))
    print("pairs with a pose:", [int(np.frombuffer(c[4], np.uint32)[-1]) for c in pose[(1, False, 2, 0, 0.99)]])
    return plain, pose


def test_bank_contents(amd, scene):
    """rows, x and y on the device against the results' descriptors padded to 64 bytes and their keypoints, byte for byte"""
    feats, padded, bank, from_sets = scene
    for b in (bank, from_sets):
        info = b.info()
        assert info["n_sets"] == 4 and info["desc_bytes"] == feats[0][1].shape[1] == 61 and info["rows"] == sum(len(k) for k, _ in feats)
        rows, x, y = b.download()
        at = 0
        for s, ((k, d), p) in enumerate(zip(feats, padded)):
            assert info["sets"][s] == dict(n_keypoints=len(k), n_descriptors=len(d), row0=at), s
            assert np.array_equal(rows[at:at + len(k)], p), s
            assert x[at:at + len(k)].tobytes() == k["x"].tobytes() and y[at:at + len(k)].tobytes() == k["y"].tobytes(), s
            at += len(k)
        assert not rows[:, 61:].any()
        assert all(b.device())


@pytest.mark.parametrize("kind", [0, 1, 3])
def test_bank_call_equals_the_sets_call(amd, ctx, scene, expected, kind):
    feats, _, bank, from_sets = scene
    for key, opt, cross in option_sets(amd, (kind,)):
        assert as_bytes(ctx.match_features_seeded_pairs(bank, PAIRS, opt, cross_check=cross)) == expected[0][key], key
        assert as_bytes(ctx.match_features_seeded_pairs(from_sets, PAIRS, opt, cross_check=cross)) == expected[0][key], ("from sets", key)
    key, opt, cross = next(option_sets(amd, (kind,)))
    assert as_bytes(amd.match_features_seeded_pairs(bank, PAIRS, opt)) == expected[0][key]  # the module-level form, on the bank's context


@pytest.mark.parametrize("kind", [1, 3])
def test_pose_bank_call_equals_the_sets_call(amd, ctx, scene, expected, kind):
    feats, _, bank, from_sets = scene
    for key, opt, cross in option_sets(amd, (kind,), guided=(0,)):
        for b in (bank, from_sets):
            assert as_bytes(ctx.match_features_seeded_pose_pairs(b, CAMERAS, PAIRS, opt, cross_check=cross, points=True)) == expected[1][key], key
    key, opt, cross = next(option_sets(amd, (kind,), guided=(0,)))
    bare = as_bytes(amd.match_features_seeded_pose_pairs(bank, CAMERAS, PAIRS, opt))
    assert bare == [row[:5] for row in expected[1][key]]


def test_model_kind_2_is_refused_alike(amd, ctx, scene):
    feats, _, bank, _ = scene
    opt = amd.RansacOptions(model_kind=2)
    for features in (feats, bank):
        with pytest.raises(amd.AkazeError) as e:
            ctx.match_features_seeded_pairs(features, PAIRS, opt)
        assert e.value.status == INVALID_ARG


def counts(amd):
    gc.collect()
    return amd.debug_resource_counts()


def test_freed_results_repeated_calls_and_no_hidden_upload(amd, ctx, expected):
    results = extract(amd, ctx)
    bank = ctx.feature_bank(results)
    for r in results:
        r.close()
    key, opt, cross = next(k for k in option_sets(amd, (1,)) if k[0] == (1, True, 2, 1, 0.99))
    before = [a.copy() for a in bank.download()]
    first = as_bytes(ctx.match_features_seeded_pairs(bank, PAIRS, opt, cross_check=cross))
    after_first = counts(amd)
    second = as_bytes(ctx.match_features_seeded_pairs(bank, PAIRS, opt, cross_check=cross))
    after_second = counts(amd)
    assert first == second == expected[0][key]
    assert all(np.array_equal(a, b) for a, b in zip(before, bank.download()))
    assert after_second["device_bytes"] <= after_first["device_bytes"] and after_second["pinned_bytes"] <= after_first["pinned_bytes"]
    bank.close()


def test_bank_call_leaves_the_upload_staging_alone(amd, scene):
    """a context that has only ever made bank calls holds less device memory than the bank's rows would need again: the sets' staging
    (rows | x | y on the device and in pinned memory) is never allocated"""
    import torch
    feats, _, _, _ = scene
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        bank = c.feature_bank(feats)
        made = counts(amd)
        opt = amd.RansacOptions(model_kind=1, max_trials=64)
        c.match_features_seeded_pairs(bank, PAIRS, opt)
        bank_calls = counts(amd)
        c.match_features_seeded_pairs(feats, PAIRS, opt)
        sets_call = counts(amd)
        assert sets_call["device_blocks"] == bank_calls["device_blocks"] + 1, (made, bank_calls, sets_call)  # mp_in, first needed now
        assert sets_call["device_bytes"] - bank_calls["device_bytes"] >= bank.info()["rows"] * 72
        bank.close()
    finally:
        c.close()


def test_one_launch_per_bank(amd, ctx):
    results = extract(amd, ctx)
    ctx.set_profiling(1)
    try:
        ctx.kernel_rows(reset=True)
        bank = ctx.feature_bank(results)
        rows = [r for r in ctx.kernel_rows() if r["kernel"] == "k_bank_gather"]
        assert len(rows) == 1 and rows[0]["launches"] == 1, rows
        assert rows[0]["n"] == 4 and rows[0]["px"] == bank.info()["rows"] and rows[0]["param"] == 61, rows
        bank.close()
    finally:
        ctx.set_profiling(0)
        for r in results:
            r.close()


@pytest.mark.parametrize("desc_bytes", [1, 15, 16, 17, 21, 41, 61, 63, 64])
def test_tail_hygiene(amd, ctx, desc_bytes):
    """hostile rows -- every byte nonzero, also beyond desc_bytes -- through the kernel: the bytes in front of desc_bytes arrive, the
    rest is zero, and nothing is written behind the last row.  301 rows: two workgroups, the second one ragged, over a table with
    an empty segment"""
    import torch
    n, guard = 301, 8
    rng = np.random.default_rng(desc_bytes)
    src = rng.integers(1, 256, (n, 64), dtype=np.uint8)
    dst = torch.full((n + guard, 64), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.debug_bank_gather(torch.from_numpy(src).cuda(), desc_bytes, dst)
    got = dst.cpu().numpy()
    assert np.array_equal(got[:n, :desc_bytes], src[:, :desc_bytes])
    assert not got[:n, desc_bytes:].any()
    assert (got[n:] == 0xA5).all()


def raw_bank_call(amd, ctx, bank_handle, pairs, opt, out=True, n_out=True, pose=False, ctx_handle=None, null_pairs=False, room=4096):
    """the ABI with every output prefilled (room: the entries of `out`) -> (status, whether every output still holds its sentinel)"""
    pr = np.ascontiguousarray(np.asarray(pairs, np.uint64).reshape(-1, 2))
    lists = np.zeros(room, amd.MATCH_DTYPE)
    lists["index_0"], lists["index_1"], lists["distance"] = 77, 78, 79.0
    n = np.full(len(pr), 12345, np.uint64)
    f = np.full((len(pr), 9), 7.0, np.float32)
    found, it, run = (np.full(len(pr), 55, t) for t in (np.int32, np.uint32, np.uint64))
    ps = np.full((len(pr), 21), 0x5A5A5A5A, np.uint32)
    pts = np.full((len(lists), 3), 9.0, np.float32)
    cams = (amd.Camera * 4)(*[amd.Camera.of(k) for k in CAMERAS])
    head = (ctx._h if ctx_handle is None else ctx_handle, bank_handle)
    rest = (None if null_pairs else pr.ctypes.data_as(C.c_void_p), len(pr), C.byref(opt) if opt is not None else None, 0,
            lists.ctypes.data_as(C.c_void_p) if out else None, n.ctypes.data_as(C.POINTER(C.c_uint64)) if n_out else None,
            f.ctypes.data_as(C.POINTER(C.c_float)), found.ctypes.data_as(C.POINTER(C.c_int32)), it.ctypes.data_as(C.POINTER(C.c_uint32)),
            run.ctypes.data_as(C.POINTER(C.c_uint64)))
    if pose:
        status = amd.lib().akz_match_features_seeded_pose_bank_pairs(*head, C.cast(cams, C.c_void_p), *rest, ps.ctypes.data_as(C.c_void_p),
                                                                     pts.ctypes.data_as(C.POINTER(C.c_float)))
    else:
        status = amd.lib().akz_match_features_seeded_bank_pairs(*head, *rest)
    untouched = (np.all(lists["index_0"] == 77) and np.all(lists["distance"] == 79.0) and np.all(n == 12345) and np.all(f == 7.0) and
                 np.all(found == 55) and np.all(it == 55) and np.all(run == 55) and np.all(ps == 0x5A5A5A5A) and np.all(pts == 9.0))
    return status, bool(untouched)


def test_refusals_come_before_any_gpu_work(amd, ctx, scene):
    import torch
    feats, _, bank, _ = scene
    opt = amd.RansacOptions(model_kind=1, max_trials=64)
    other = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    room = sum(bank.info()["sets"][a]["n_descriptors"] for a, _ in PAIRS) + 16
    assert raw_bank_call(amd, ctx, bank._h, PAIRS, opt, room=room)[0] == 0  # (the good call, so that every buffer it needs is there)
    results = extract(amd, ctx)
    one_channel = ctx.extract_features(torch.from_numpy(frames(amd)[1]).cuda(), amd.Config(descriptor_channels=1), keep_all_planes=False)
    start = counts(amd)
    try:
        for pose in (False, True):
            cases = dict(null_bank=dict(bank_handle=None, pairs=PAIRS, opt=opt), null_pairs=dict(bank_handle=bank._h, pairs=PAIRS, opt=opt, null_pairs=True),
                         null_context=dict(bank_handle=bank._h, pairs=PAIRS, opt=opt, ctx_handle=C.c_void_p()),
                         null_options=dict(bank_handle=bank._h, pairs=PAIRS, opt=None),
                         null_n_out=dict(bank_handle=bank._h, pairs=PAIRS, opt=opt, n_out=False),
                         null_out_with_room_needed=dict(bank_handle=bank._h, pairs=PAIRS, opt=opt, out=False),
                         set_index_beyond_the_bank=dict(bank_handle=bank._h, pairs=[(0, 2), (2, 4)], opt=opt),
                         bank_of_another_context=dict(bank_handle=bank._h, pairs=PAIRS, opt=opt, ctx_handle=other._h))
            for name, kw in cases.items():
                status, untouched = raw_bank_call(amd, ctx, pose=pose, room=room, **kw)
                assert status == INVALID_ARG and untouched, (name, pose, status, untouched)
                assert amd.lib().akz_last_error(), name
        assert "another context" in _message(amd, lambda: raw_bank_call(amd, ctx, bank._h, PAIRS, opt, ctx_handle=other._h))
        assert "set index 4 >= n_sets 4" in _message(amd, lambda: raw_bank_call(amd, ctx, bank._h, [(0, 2), (2, 4)], opt))
        # creation: null arguments, descriptor sizes that differ
        h = C.c_void_p(0xdead)
        arr = (C.c_void_p * 2)(results[0]._h, one_channel._h)
        assert amd.lib().akz_bank_create_from_results(ctx._h, arr, 2, C.byref(h)) == INVALID_ARG and h.value is None
        assert "bytes" in amd.lib().akz_last_error().decode()
        with pytest.raises(amd.AkazeError, match="result 1: descriptors of 21 bytes, result 0 has 61"):
            ctx.feature_bank([results[1], one_channel])
        arr = (C.c_void_p * 2)(results[0]._h, None)
        assert amd.lib().akz_bank_create_from_results(ctx._h, arr, 2, C.byref(h)) == INVALID_ARG
        assert amd.lib().akz_bank_create_from_results(None, arr, 1, C.byref(h)) == INVALID_ARG
        assert amd.lib().akz_bank_create_from_results(ctx._h, None, 1, C.byref(h)) == INVALID_ARG
        assert amd.lib().akz_bank_create_from_results(ctx._h, arr, 1, None) == INVALID_ARG
        assert amd.lib().akz_bank_create_from_results(ctx._h, arr, 0, C.byref(h)) == INVALID_ARG
        assert counts(amd) == start
    finally:
        other.close()
        one_channel.close()
        for r in results:
            r.close()


def _message(amd, call):
    call()
    return amd.lib().akz_last_error().decode()


def test_resources_come_back(amd):
    """in the style of test_gpu_ctx_resources.py: the counters rise when a bank is made and are where they were after close() and the
    context's destruction -- and, in the other order, a bank that outlives its context keeps exactly its one block, is refused by
    every call, and gives the block back when it is closed"""
    import torch
    before = counts(amd)
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    results = extract(amd, c)
    feats = host_sets(results)
    idle = counts(amd)
    bank = c.feature_bank(results)
    made = counts(amd)
    # (two blocks on a context that has matched nothing yet: the bank's, and the context's scratch that the segment table passes through)
    assert made["device_blocks"] == idle["device_blocks"] + 2 and made["device_bytes"] >= idle["device_bytes"] + bank.info()["rows"] * 72, (idle, made)
    again = c.feature_bank(feats)
    assert counts(amd)["device_blocks"] == made["device_blocks"] + 1
    c.match_features_seeded_pairs(bank, PAIRS, amd.RansacOptions(max_trials=64))
    busy = counts(amd)
    bank.close()
    again.close()
    left = counts(amd)  # closing a bank gives back its one block, and nothing of the context's
    assert left["device_blocks"] == busy["device_blocks"] - 2 and busy["device_bytes"] - left["device_bytes"] >= 2 * 72 * sum(len(k) for k, _ in feats)
    assert all(left[k] == busy[k] for k in ("pinned_blocks", "pinned_bytes", "events", "streams")), (busy, left)
    for r in results:
        r.close()
    c.close()
    assert counts(amd) == before, {k: counts(amd)[k] - before[k] for k in before}
    # the context goes first
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    bank = c.feature_bank(feats)
    c.match_features_seeded_pairs(bank, PAIRS, amd.RansacOptions(max_trials=64))
    h = c._h
    c.close()
    mid = counts(amd)
    assert mid["device_blocks"] == before["device_blocks"] + 1 and all(mid[k] == before[k] for k in ("pinned_blocks", "pinned_bytes", "events", "streams")), (before, mid)
    c._h = h  # (the struct lives as long as the bank: the call reaches the library and is refused there)
    try:
        with pytest.raises(amd.AkazeError, match="context of this object was destroyed"):
            c.match_features_seeded_pairs(bank, PAIRS, amd.RansacOptions(max_trials=64))
    finally:
        c._h = C.c_void_p()
    assert bank.info()["n_sets"] == 4
    bank.close()
    assert counts(amd) == before
