"""The feature bank under a keypoint budget on the GPU (akz_bank_create_from_results_budget / _from_sets_budget, akz_bank_set_indices,
k_bank_select; include/akaze_hip.h).

The statement: set s of a budgeted bank is (K_s[idx_s], D_s[idx_s]) with idx_s = keypoint_budget_host(K_s, N, mode, robust), and the
bank is byte for byte the bank of those sliced host sets.  The scene is that of test_gpu_feature_bank.py: 320 x 240 synthetic
frames that are shifted copies of one another and one flat frame, which gives a set of 0 keypoints; two results, a batch of three
and a lone one, give four sets.  N comes from the scene's own counts.  Every reference is computed once from the results' host
copies and left unchanged; everything is compared as bytes."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 320, 240
INVALID_ARG = -1
PAIRS = [(0, 2), (0, 2), (2, 0), (0, 0), (1, 0), (0, 1), (2, 3), (0, 3)]
RELATED = (0, 1, 2, 6, 7)  # the pairs of PAIRS between two frames that show the same scene
EPSILON = {0: 3.0, 1: 0.02, 3: 2.0}  # pixels for a homography, the algebraic residual at unit norm, Sampson pixels
BASE = (1 << 64) - 3              # the pairs' streams wrap around
CAMERAS = [(400.0 + 3 * s, 400.0 - 2 * s, 160.0 + s, 120.0 - s) for s in range(4)]
ROBUST = 0.9


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


def sliced(amd, feats, n, mode):
    """the statement on the host -> ([idx per set], [(K[idx], D[idx]) per set])"""
    idx = [amd.keypoint_budget_host(k, n, mode, ROBUST)[0] for k, _ in feats]
    return idx, [(np.ascontiguousarray(k[i]), np.ascontiguousarray(d[i])) for (k, d), i in zip(feats, idx)]


def snapshot(bank):
    """everything a bank shows, as bytes: info, rows | x | y on the device, the source indices of every set"""
    rows, x, y = bank.download()
    return bank.info(), rows.tobytes(), x.tobytes(), y.tobytes(), [(i.dtype.str, i.tobytes()) for i in bank.indices()]


@pytest.fixture(scope="module")
def scene(amd, ctx):
    """host sets, the budgets of the scene, and for every (N, mode) the snapshot of feature_bank(results, budget) -- taken after the
    results were closed -- and the two banks the downstream tests use"""
    results = extract(amd, ctx)
    feats = host_sets(results)
    counts = [len(k) for k, _ in feats]
    assert counts[1] == 0 and min(counts[0], counts[2], counts[3]) >= 16, counts
    n_mixed = min(counts[0], counts[2], counts[3])  # the smallest non-empty set is kept whole, every larger one is cut
    assert max(counts) > n_mixed, counts
    budgets = [(n_mixed, amd.BUDGET_SPREAD), (n_mixed, amd.BUDGET_STRONGEST), (n_mixed // 2, amd.BUDGET_SPREAD), (n_mixed // 2, amd.BUDGET_STRONGEST),
               (max(counts) + 5, amd.BUDGET_SPREAD), (0, amd.BUDGET_SPREAD)]
    banks = {b: ctx.feature_bank(results, budget=amd.KeypointBudget(b[0], b[1], ROBUST)) for b in budgets}
    plain = ctx.feature_bank(results)
    for r in results:
        r.close()
    gc.collect()
    shots = {b: snapshot(bank) for b, bank in banks.items()}
    shots["plain"] = snapshot(plain)
    plain.close()
    yield dict(feats=feats, counts=counts, n=n_mixed, budgets=budgets, banks=banks, shots=shots)
    for bank in banks.values():
        bank.close()


def expected_snapshot(amd, feats, n, mode):
    """what the statement says a budgeted bank shows, built with numpy from the host copies"""
    idx, cut = sliced(amd, feats, n, mode)
    sets, at = [], 0
    for k, _ in cut:
        sets.append(dict(n_keypoints=len(k), n_descriptors=len(k), row0=at))
        at += len(k)
    info = dict(n_sets=len(cut), desc_bytes=61, rows=at, sets=sets)
    rows = np.concatenate([np.pad(d.reshape(-1, 61), ((0, 0), (0, 3))) for _, d in cut])
    x = np.concatenate([k["x"] for k, _ in cut]).astype(np.float32)
    y = np.concatenate([k["y"] for k, _ in cut]).astype(np.float32)
    return info, rows.tobytes(), x.tobytes(), y.tobytes(), [(i.astype(np.uint64).dtype.str, i.astype(np.uint64).tobytes()) for i in idx]


def test_bank_contents(amd, ctx, scene):
    feats, counts, n = scene["feats"], scene["counts"], scene["n"]
    assert feats[0][1].shape[1] == 61
    for n_keep, mode in scene["budgets"][:4]:
        idx, cut = sliced(amd, feats, n_keep, mode)
        kept = [len(i) for i in idx]
        assert kept == [min(n_keep, c) for c in counts] and kept[1] == 0, (kept, counts)
        if n_keep == n:  # the budget does its job on this scene: a non-empty set is cut, another is kept whole
            assert any(0 < k < c for k, c in zip(kept, counts)) and any(0 < k == c for k, c in zip(kept, counts)), (kept, counts)
        else:
            assert all(k < c for k, c in zip(kept, counts) if c), (kept, counts)
        want = expected_snapshot(amd, feats, n_keep, mode)
        assert scene["shots"][(n_keep, mode)] == want, (n_keep, mode)
        budget = amd.KeypointBudget(n_keep, mode, ROBUST)
        for name, make in (("bank of the sliced host sets", lambda: ctx.feature_bank(cut)),
                           ("budgeted bank of the host sets", lambda: ctx.feature_bank(feats, budget=budget))):
            bank = make()
            got = snapshot(bank)
            bank.close()
            if name.startswith("bank of"):  # (a bank made without a budget names its own rows)
                assert got[:4] == want[:4] and got[4] == [("<u8", np.arange(k, dtype=np.uint64).tobytes()) for k in kept], (name, n_keep, mode)
            else:
                assert got == want, (name, n_keep, mode)
    # the two modes do not keep the same keypoints here, so neither stands in for the other
    assert scene["shots"][(n // 2, amd.BUDGET_SPREAD)][4] != scene["shots"][(n // 2, amd.BUDGET_STRONGEST)][4]


def test_identity_and_nothing(amd, ctx, scene):
    feats, counts = scene["feats"], scene["counts"]
    whole = scene["shots"][(max(counts) + 5, amd.BUDGET_SPREAD)]
    assert whole[:4] == scene["shots"]["plain"][:4]
    assert whole[4] == scene["shots"]["plain"][4] == [("<u8", np.arange(c, dtype=np.uint64).tobytes()) for c in counts]
    bank = ctx.feature_bank(feats, budget=amd.KeypointBudget(max(counts), amd.BUDGET_STRONGEST, ROBUST))
    assert snapshot(bank) == whole
    bank.close()
    info, rows, x, y, idx = scene["shots"][(0, amd.BUDGET_SPREAD)]
    empty = dict(n_keypoints=0, n_descriptors=0, row0=0)
    assert info == dict(n_sets=4, desc_bytes=61, rows=0, sets=[empty] * 4) and rows == x == y == b"" and idx == [("<u8", b"")] * 4
    nothing = scene["banks"][(0, amd.BUDGET_SPREAD)]
    from_sets = ctx.feature_bank(feats, budget=amd.KeypointBudget(0, amd.BUDGET_STRONGEST, ROBUST))
    assert snapshot(from_sets) == scene["shots"][(0, amd.BUDGET_SPREAD)]
    no_sets = [(k[:0], d[:0]) for k, d in feats]
    for cross in (False, True):
        opt = amd.RansacOptions(model_kind=1, max_trials=64, refine_iterations=2)
        want = as_bytes(ctx.match_features_seeded_pairs(no_sets, PAIRS, opt, cross_check=cross))
        for bank in (nothing, from_sets):
            got = ctx.match_features_seeded_pairs(bank, PAIRS, opt, cross_check=cross)
            assert all(len(row[0]) == 0 and row[1] is None for row in got)  # empty lists, found = 0
            assert as_bytes(got) == want
    from_sets.close()


def option_sets(amd, kinds, guided=(0, 1)):
    for kind, cross, its, g in itertools.product(kinds, (False, True), (0, 2), guided):
        opt = amd.RansacOptions(model_kind=kind, max_trials=256, confidence=0.99, refine_iterations=its, epsilon_inliers=EPSILON[kind],
                                stream_base=BASE, guided=g, guided_radius=3.0, guided_lowes_ratio=0.9)
        yield (kind, cross, its, g), opt, cross


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


@pytest.fixture(scope="module")
def downstream(amd, ctx, scene):
    """the sets calls over the SLICED host copies (SPREAD, the scene's N), computed once, and the two budgeted banks held to them"""
    feats, n = scene["feats"], scene["n"]
    _, cut = sliced(amd, feats, n, amd.BUDGET_SPREAD)
    plain = {key: as_bytes(ctx.match_features_seeded_pairs(cut, PAIRS, opt, cross_check=cross)) for key, opt, cross in option_sets(amd, (0, 1, 3))}
    pose = {key: as_bytes(ctx.match_features_seeded_pose_pairs(cut, CAMERAS, PAIRS, opt, cross_check=cross, points=True))
            for key, opt, cross in option_sets(amd, (1, 3), guided=(0,))}
    # at this N related pairs still find a model, and pairs with an empty set keep nothing
    for kind in (0, 1, 3):
        found = [plain[(kind, False, 2, 0)][p][1] is not None for p in range(len(PAIRS))]
        assert any(found[p] for p in RELATED) and not found[4] and not found[5], (kind, found)
    assert any(pose[(1, False, 2, 0)][p][1] is not None for p in RELATED)
    from_sets = ctx.feature_bank(feats, budget=amd.KeypointBudget(n, amd.BUDGET_SPREAD, ROBUST))
    yield plain, pose, (scene["banks"][(n, amd.BUDGET_SPREAD)], from_sets)
    from_sets.close()


@pytest.mark.parametrize("kind", [0, 1, 3])
def test_bank_call_equals_the_sets_call_over_the_sliced_sets(amd, ctx, downstream, kind):
    plain, _, banks = downstream
    for key, opt, cross in option_sets(amd, (kind,)):
        for bank in banks:
            assert as_bytes(ctx.match_features_seeded_pairs(bank, PAIRS, opt, cross_check=cross)) == plain[key], key


@pytest.mark.parametrize("kind", [1, 3])
def test_pose_bank_call_equals_the_sets_call_over_the_sliced_sets(amd, ctx, downstream, kind):
    _, pose, banks = downstream
    for key, opt, cross in option_sets(amd, (kind,), guided=(0,)):
        for bank in banks:
            assert as_bytes(ctx.match_features_seeded_pose_pairs(bank, CAMERAS, PAIRS, opt, cross_check=cross, points=True)) == pose[key], key


# ---- the kernel alone -------------------------------------------------------------------------------------------------
SEL_N, SEL_KEEP, GUARD = (301, 0, 700), (130, 0, 257), 8


def select_inputs():
    """hostile sources -- every byte nonzero, also beyond desc_bytes -- and a seeded ascending subset per set with index 0 and n - 1"""
    rng = np.random.default_rng(31)
    total = sum(SEL_N)
    src = rng.integers(1, 256, (total, 64), dtype=np.uint8)
    sx, sy = rng.random(total, dtype=np.float32) * 320, rng.random(total, dtype=np.float32) * 240
    idx = []
    for n, keep in zip(SEL_N, SEL_KEEP):
        if keep:
            inner = rng.choice(np.arange(1, n - 1), keep - 2, replace=False)
            idx.append(np.sort(np.concatenate([[0, n - 1], inner])).astype(np.uint32))
        else:
            idx.append(np.zeros(0, np.uint32))
    return src, sx, sy, idx


def run_select(ctx, src, sx, sy, idx, desc_bytes, n=SEL_N, keep=SEL_KEEP):
    """-> (rows, x, y, index) as uint8 arrays, guards included; every destination prefilled with 0xA5"""
    import torch
    rows = sum(SEL_KEEP) + GUARD
    dst = [torch.full((rows * width,), 0xA5, dtype=torch.uint8, device="cuda") for width in (64, 4, 4, 4)]
    dev = [torch.from_numpy(a).cuda() for a in (src, sx, sy)]
    try:
        ctx.debug_bank_select(*dev, n, keep, np.concatenate(idx) if len(idx) else np.zeros(0, np.uint32), desc_bytes, *dst)
    finally:
        torch.cuda.synchronize()
    return [d.cpu().numpy() for d in dst]


@pytest.mark.parametrize("desc_bytes", [1, 15, 16, 17, 21, 41, 61, 63, 64])
def test_kernel_alone(amd, ctx, desc_bytes):
    """387 destination rows: two workgroups, the second one ragged, a set boundary inside the first and an empty set between the
    other two.  The bytes in front of desc_bytes equal the indexed source, the rest is zero; x, y and the index equal the indexed
    source; nothing behind the last row is written"""
    src, sx, sy, idx = select_inputs()
    kept = sum(SEL_KEEP)
    assert kept == 387 and all(len(i) == k for i, k in zip(idx, SEL_KEEP)) and idx[0][0] == 0 and idx[0][-1] == 300 and idx[2][-1] == 699
    base = np.cumsum((0,) + SEL_N)[:3]
    flat = np.concatenate([b + i.astype(np.int64) for b, i in zip(base, idx)])  # the source row of every destination row
    rows, x, y, index = run_select(ctx, src, sx, sy, idx, desc_bytes)
    rows = rows.reshape(-1, 64)
    assert np.array_equal(rows[:kept, :desc_bytes], src[flat, :desc_bytes])
    assert not rows[:kept, desc_bytes:].any()
    assert (rows[kept:] == 0xA5).all()
    assert x[:kept * 4].tobytes() == sx[flat].tobytes() and y[:kept * 4].tobytes() == sy[flat].tobytes()
    assert index[:kept * 4].tobytes() == np.concatenate(idx).astype(np.uint32).tobytes()
    for tail in (x, y, index):
        assert (tail[kept * 4:] == 0xA5).all()


def test_kernel_hook_refuses_bad_index_lists(amd, ctx):
    src, sx, sy, idx = select_inputs()
    swapped = [i.copy() for i in idx]
    swapped[2][[5, 6]] = swapped[2][[6, 5]]
    repeated = [i.copy() for i in idx]
    repeated[0][9] = repeated[0][8]
    beyond = [i.copy() for i in idx]
    beyond[0][-1] = SEL_N[0]
    for name, bad, word in (("not ascending", swapped, "set 2"), ("repeated", repeated, "set 0"), ("reaches n", beyond, "set 0")):
        with pytest.raises(amd.AkazeError, match=word) as e:
            run_select(ctx, src, sx, sy, bad, 61)
        assert e.value.status == INVALID_ARG, name
    with pytest.raises(amd.AkazeError, match="set 2"):  # more kept than there are
        run_select(ctx, src, sx, sy, idx, 61, keep=(130, 0, 701))
    # nothing was launched: the same destinations, handed to a refused call, keep their fill
    import torch
    dst = [torch.full(((387 + GUARD) * width,), 0xA5, dtype=torch.uint8, device="cuda") for width in (64, 4, 4, 4)]
    dev = [torch.from_numpy(a).cuda() for a in (src, sx, sy)]
    with pytest.raises(amd.AkazeError):
        ctx.debug_bank_select(*dev, SEL_N, SEL_KEEP, np.concatenate(beyond), 61, *dst)
    torch.cuda.synchronize()
    assert all(bool((d == 0xA5).all()) for d in dst)


# ---- launches, refusals, resources ------------------------------------------------------------------------------------
def counts(amd):
    gc.collect()
    return amd.debug_resource_counts()


def test_one_launch_per_budgeted_bank(amd, ctx, scene):
    results = extract(amd, ctx)
    ctx.set_profiling(1)
    try:
        for source in (results, scene["feats"]):
            ctx.kernel_rows(reset=True)
            bank = ctx.feature_bank(source, budget=amd.KeypointBudget(scene["n"], amd.BUDGET_SPREAD, ROBUST))
            rows = ctx.kernel_rows()
            select = [r for r in rows if r["kernel"] == "k_bank_select"]
            assert len(select) == 1 and select[0]["launches"] == 1, rows
            assert select[0]["n"] == 4 and select[0]["px"] == bank.info()["rows"] == sum(min(scene["n"], c) for c in scene["counts"]), select
            assert select[0]["param"] == 61, select
            assert not [r for r in rows if r["kernel"] == "k_bank_gather"], rows
            bank.close()
    finally:
        ctx.set_profiling(0)
        for r in results:
            r.close()


def test_refusals_come_before_any_gpu_work(amd, ctx, scene):
    import torch
    L = amd.lib()
    results = extract(amd, ctx)
    one_channel = ctx.extract_features(torch.from_numpy(frames(amd)[1]).cuda(), amd.Config(descriptor_channels=1), keep_all_planes=False)
    good = amd.KeypointBudget(scene["n"], amd.BUDGET_SPREAD, ROBUST)
    ctx.feature_bank(results, budget=good).close()  # (the good call, so that every buffer it needs is there)
    start = counts(amd)
    try:
        both = (C.c_void_p * 2)(results[0]._h, results[1]._h)
        cases = dict(null_budget=(both, 2, None, "null options"), bad_mode=(both, 2, amd.KeypointBudget(5, 9, ROBUST), "unknown mode 9"),
                     bad_robust=(both, 2, amd.KeypointBudget(5, amd.BUDGET_SPREAD, 1.5), "robust"),
                     differing_descriptor_sizes=((C.c_void_p * 2)(results[0]._h, one_channel._h), 2, good, "result 1: descriptors of 21 bytes, result 0 has 61"),
                     null_result=((C.c_void_p * 2)(results[0]._h, None), 2, good, "result 1: null"),
                     no_result=(both, 0, good, "no result"), null_results=(None, 1, good, "null"))
        for name, (arr, n, budget, word) in cases.items():
            h = C.c_void_p(0xdead)
            status = L.akz_bank_create_from_results_budget(ctx._h, arr, n, C.byref(budget) if budget is not None else None, C.byref(h))
            assert status == INVALID_ARG and h.value is None and word in L.akz_last_error().decode(), (name, status, L.akz_last_error().decode())
        assert L.akz_bank_create_from_results_budget(ctx._h, both, 2, C.byref(good), None) == INVALID_ARG
        h = C.c_void_p(0xdead)
        assert L.akz_bank_create_from_results_budget(None, both, 2, C.byref(good), C.byref(h)) == INVALID_ARG and h.value is None
        # (a result is unfinished only inside a job, which hands none out: the NULL result stands for both)
        # a keypoint that is not finite, from host sets: the message names the set
        feats = [(k.copy(), d) for k, d in scene["feats"]]
        feats[2][0]["response"][3] = np.nan
        with pytest.raises(amd.AkazeError, match="set 2: keypoint 3") as e:
            ctx.feature_bank(feats, budget=good)
        assert e.value.status == INVALID_ARG
        assert counts(amd) == start
    finally:
        one_channel.close()
        for r in results:
            r.close()


def test_resources_come_back(amd, scene):
    """in the style of test_gpu_feature_bank.py: a budgeted bank owns exactly one device block, close() returns exactly that block,
    the context's destruction the rest -- and a budgeted bank that outlives its context keeps its one block and is refused"""
    import torch
    before = counts(amd)
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    results = extract(amd, c)
    feats = host_sets(results)
    budget = amd.KeypointBudget(scene["n"], amd.BUDGET_SPREAD, ROBUST)
    kept = sum(min(scene["n"], n) for n in scene["counts"])
    idle = counts(amd)
    bank = c.feature_bank(results, budget=budget)
    made = counts(amd)
    # (three blocks on a context that has matched nothing yet: the bank's, the budget's scratch, and the scratch the table passes through)
    assert made["device_blocks"] == idle["device_blocks"] + 3 and made["device_bytes"] >= idle["device_bytes"] + kept * 76, (idle, made)
    second = c.feature_bank(results, budget=budget)  # every scratch is there now: the bank's one block
    assert counts(amd)["device_blocks"] == made["device_blocks"] + 1
    again = c.feature_bank(feats, budget=budget)  # its block, and the staging the full sets pass through
    assert counts(amd)["device_blocks"] == made["device_blocks"] + 3
    c.match_features_seeded_pairs(bank, PAIRS, amd.RansacOptions(max_trials=64))
    busy = counts(amd)
    for b in (bank, second, again):
        b.close()
    left = counts(amd)  # closing a bank gives back its one block, and nothing of the context's
    assert left["device_blocks"] == busy["device_blocks"] - 3 and busy["device_bytes"] - left["device_bytes"] >= 3 * 76 * kept
    assert busy["device_bytes"] - left["device_bytes"] <= 3 * (76 * kept + 4 * 256)
    assert all(left[k] == busy[k] for k in ("pinned_blocks", "pinned_bytes", "events", "streams")), (busy, left)
    for r in results:
        r.close()
    c.close()
    assert counts(amd) == before, {k: counts(amd)[k] - before[k] for k in before}
    # the context goes first
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    bank = c.feature_bank(feats, budget=budget)
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
    assert bank.info()["n_sets"] == 4 and [len(i) for i in bank.indices()] == [min(scene["n"], n) for n in scene["counts"]]
    bank.close()
    assert counts(amd) == before
