"""What a context owns is released with it: device blocks, pinned blocks, events and streams, read through
akz_debug_resource_counts -- the owning types' own process-wide counters.  Every case reads the counters, creates a context of its
own, runs a workload, asserts that the counters rose (device bytes, and an event or a stream: no vacuous pass), frees the results,
destroys the context and asserts that all six counters are where they were.  A member of the context that nobody releases shows as
a difference in the case whose workload allocates it.

The counters are the code under test's own, so one case checks against the runtime instead: free device memory as
torch.cuda.mem_get_info() reports it does not drift over create / use / destroy cycles by more than it did on the parent commit's
build (measured once: PARENT_MAX_DRIFT_BYTES).  That case also runs on a library without the hook (AKAZE_HIP_LIB and the binding
that goes with it), where the counter asserts are left out."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

from test_gpu_pairs_front_tail import EPS, ITS, PAIRS, RADIUS, RATIO, TRIALS, build_sets, seeded_options
from test_gpu_scratch_claims import audit, match_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
# The parent commit's build, create / three host jobs / destroy five times in a process of its own (one MI355X, round 25;
# CHANGELOG.md): free device memory after cycles 1 .. 5 was 308 254 081 024, then 308 145 029 120 four times -- the runtime settles
# during the second cycle of a fresh process (104 MiB, once), and from cycle 2 to cycle 5 no cycle loses a byte.
PARENT_MAX_DRIFT_BYTES = 0


def counts(amd):
    """the six counters, or None on a library without the hook"""
    gc.collect()  # (a result or a context that an earlier test dropped without closing goes now, not in the middle of a case)
    read = getattr(amd, "debug_resource_counts", None)
    return read() if read else None


def fresh_context(amd):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return amd.Context(0, torch.cuda.current_stream().cuda_stream)


def frames(amd, w, h, n, first=0, device=True):
    import torch
    t = torch.from_numpy(np.stack([amd.synth_frame(w, h, first + i) for i in range(n)]))
    return t.cuda() if device else t.pin_memory()


def accounted(amd, workload, rises=True):
    """workload(context) on a context of its own -> whatever it returns; the counters rise and come back"""
    before = counts(amd)
    c = fresh_context(amd)
    try:
        out = workload(c)
        during = counts(amd)
    finally:
        c.close()
    after = counts(amd)
    if before is not None:
        if rises:
            assert during["device_bytes"] > before["device_bytes"] and during["device_blocks"] > before["device_blocks"], (before, during)
            assert during["events"] > before["events"] or during["streams"] > before["streams"], (before, during)
        assert after == before, {k: after[k] - before[k] for k in KINDS}
    return out


def test_create_and_destroy(amd):
    accounted(amd, lambda c: None, rises=False)


def test_lone_extraction_profiled_and_its_fetches(amd):
    """spans and the event pool (profiling of every stage); fetch_pyramid: the fetch streams, events and the pinned staging; a plane
    of a lean result: `lazy` and the recomputation's temporaries"""
    d = frames(amd, 640, 360, 1)

    def workload(c):
        c.set_profiling(1)
        full = c.extract_features(d, keep_all_planes=True)
        assert len(full.pyramid(0)) == len(amd.plan_levels(640, 360))
        lean = c.extract_features(d, keep_all_planes=False)
        assert lean.plane(1, "Lxx").size > 0 and len(lean.pyramid(0)) > 0
        c.get_profile()
        n = len(full.keypoints(0))
        full.close()
        lean.close()
        return n

    assert accounted(amd, workload) > 0


def host_jobs(amd, c, host):
    """three jobs of 4 frames from pinned host memory on the batch path, begun back to back (every slot's staging buffer and
    event, the copy stream, fed_ev / pre_ev, the fork's coarse stream) with the early stages on a stream of their own (`pre`), under
    eager finish (the finisher thread, the auxiliary stream)"""
    c.set_eager_finish(True)
    c.debug_set_schedule(4, 1)  # SCHED_JOB_KPX: every job takes the batch path
    c.debug_set_schedule(6, 1)  # SCHED_PREP_OWN_LAUNCH: the automatic preparation, which is what runs ahead
    c.debug_set_schedule(0, 2)  # SCHED_EARLY_STREAM: a stream of their own
    jobs = [c.extract_begin_host(h, keep_all_planes=False) for h in host]
    res = [j.finish() for j in jobs]
    kp = [len(r.keypoints(i)) for r in res for i in range(4)]
    for r in res:
        r.close()
    return kp


def test_three_host_jobs_in_flight(amd):
    host = [frames(amd, 640, 360, 4, 4 * b, device=False) for b in range(3)]
    kp = accounted(amd, lambda c: host_jobs(amd, c, host))
    assert len(kp) == 12 and min(kp) > 0


def test_lanes_shrunk_and_destroyed(amd):
    """lane teardown is both akz_ctx_set_lanes shrinking and akz_ctx_destroy"""
    d = [frames(amd, 640, 360, 1, i) for i in range(4)]

    def small_jobs(c):
        jobs = [c.extract_begin(f, keep_all_planes=False) for f in d[:3]]
        res = [j.finish() for j in jobs] + [c.extract_begin(d[3], keep_all_planes=False).finish()]
        kp = [len(r.keypoints(0)) for r in res]
        for r in res:
            r.close()
        return kp

    def shrunk(c):  # (the context itself runs nothing: what rose is the lanes', and shrinking gives it back)
        idle = counts(amd)
        c.set_lanes(2)
        kp = small_jobs(c)
        busy = counts(amd)
        c.set_lanes(1)
        assert busy["device_bytes"] > idle["device_bytes"] and busy["streams"] >= idle["streams"] + 2, (idle, busy)
        left = counts(amd)  # (the context's own events stay until it goes: lane_in and the two of place_lanes' probe)
        assert all(left[k] == idle[k] for k in KINDS if k != "events") and left["events"] == idle["events"] + 3, (idle, left)
        return kp

    def destroyed_with_lanes(c):
        c.set_lanes(2)
        return small_jobs(c)

    kp = accounted(amd, shrunk, rises=False)
    assert kp == accounted(amd, destroyed_with_lanes) and min(kp) > 0


def test_stream_placement_probe(amd):
    """a job on the batch path runs the probe first; streams it replaces must not stay behind"""
    d = frames(amd, 640, 360, 1)

    def workload(c):
        c.debug_set_schedule(4, 1)
        r = c.extract_begin(d, keep_all_planes=False).finish()
        n = len(r.keypoints(0))
        r.close()
        assert c.debug_stream_placement()["probed"]
        return n

    assert accounted(amd, workload) > 0


def test_jpeg_ingest(amd):
    def workload(c):
        r = c.extract_features_file(os.path.join(ROOT, "tests", "golden", "1.jpg"), keep_all_planes=False)
        n = len(r.keypoints(0))
        r.close()
        return n

    assert accounted(amd, workload) > 0


def test_matchers(amd):
    """descriptor_match under the three matcher modes (2048 query rows: the merging compaction and its state), the multi-set and the
    mutual call on side 0, and akz_match_all_pairs over three images, which alternates the sides"""
    import torch
    d0, d1 = match_sets(2048, 1300, 4)
    q = torch.from_numpy(np.pad(d0, ((0, 0), (0, 3)))).cuda()
    t = torch.from_numpy(np.pad(d1, ((0, 0), (0, 3)))).cuda()
    three = frames(amd, 320, 240, 3)

    def workload(c):
        lists = []
        for mode in (0, 1, 2):
            c.set_match_mode(mode)
            lists.append(c.descriptor_match(d0, d1, 10000, 0.86))
        assert len(lists[0]) == 512 and all(np.array_equal(m, lists[0]) for m in lists)
        _, cnt = c.descriptor_match_sets_device(q, t, [650, 650])
        _, cnt2, _, ccnt = c.descriptor_match_sets_mutual_device(q, t, [650, 650])
        c.synchronize()
        assert int(cnt.sum()) == int(cnt2.sum()) >= 512 and int(ccnt.sum()) > 0  # (every planted row passes in its own set)
        res = c.extract_features(three, keep_all_planes=False)
        rows = sum(res.counts(i)[1] for i in range(3))
        comm = amd.Comm(0, amd.comm_unique_id(), 0, 1)  # (the communicator's own objects are not the context's and not counted)
        g = comm.gather_begin([res], rows + 1)
        pairs = g.match_all_pairs(c)
        total = pairs.total_matches()
        pairs.free()
        g.free()
        comm.close()
        res.close()
        return total

    assert accounted(amd, workload) > 0


def test_pairs_calls(amd):
    """the pairs calls: plain, homography refined + guided, fundamental, seeded, seeded and cross-checked; kNN; the keypoint budget;
    with the split timing of the pairs calls and of the budget on (their events)"""
    sets = build_sets(amd)

    def workload(c):
        ms = (C.c_double * 6)()
        assert amd.lib().akz_debug_match_pairs_split(c._h, 1, ms) == 0
        c.debug_keypoint_budget_split(True)
        amd.random_seed(42, 69)
        n = [len(m) for m in c.match_features_pairs(sets, PAIRS, RATIO, TRIALS, 0.02)]
        n += [len(g[0]) for g in c.match_features_homography_refined_guided_pairs(sets, PAIRS, RATIO, TRIALS, EPS, ITS, RADIUS, RATIO)]
        n += [len(g[0]) for g in c.match_features_fundamental_pairs(sets, PAIRS, RATIO, TRIALS, 0.02)]
        opt = seeded_options(amd, 0.99, guided=1, guided_radius=RADIUS, guided_lowes_ratio=RATIO)
        n += [len(g[0]) for g in c.match_features_seeded_pairs(sets, PAIRS, opt)]
        n += [len(g[0]) for g in c.match_features_seeded_pairs(sets, PAIRS, opt, cross_check=True)]
        recs, cnt = c.descriptor_match_knn(sets[0][1], sets[1][1], 2, 120)
        n.append(int(cnt.sum()))
        kept = c.keypoint_budget_sets(sets[:3], 100)
        n += [len(k[0]) for k in kept]
        return n

    n = accounted(amd, workload)
    assert n[4 + 0] > 150 and 0 < n[-1] <= 100, n  # (the guided list of the first, related pair; the budget of a 300-keypoint set)


def test_growth_releases_what_it_replaces(amd):
    """a small job, a larger one, the small one again on one context: every scratch buffer the larger job outgrew was freed when it
    was replaced, so the third job adds no block; the scratch claims hold after each"""
    small, large = frames(amd, 320, 240, 1), frames(amd, 640, 480, 2)

    def workload(c):
        c.debug_set_alloc_fill(True)
        blocks = []
        for step, d in enumerate((small, large, small)):
            r = c.extract_features(d, keep_all_planes=False)
            audit(c, step)
            assert len(r.keypoints(0)) > 0
            r.close()
            now = counts(amd)
            blocks.append(now and now["device_blocks"])
        assert blocks[2] == blocks[1], blocks
        return blocks

    accounted(amd, workload)


def test_context_destroyed_before_its_result(amd):
    """the "wrong" order: the context's resources go with akz_ctx_destroy, the result keeps its own blocks and nothing else, a
    fetch on it is refused, and freeing it brings the rest back"""
    d = frames(amd, 640, 360, 1)
    before = counts(amd)
    c = fresh_context(amd)
    res = c.extract_features(d, keep_all_planes=False)
    c.close()
    mid = counts(amd)
    with pytest.raises(amd.AkazeError, match="context of this object was destroyed"):
        res.plane(0, "Lt")
    res.close()
    after = counts(amd)
    assert before is not None
    assert all(mid[k] == before[k] for k in ("pinned_blocks", "pinned_bytes", "events", "streams")), (before, mid)
    assert 1 <= mid["device_blocks"] - before["device_blocks"] <= 2 and mid["device_bytes"] > before["device_bytes"], (before, mid)
    assert after == before, {k: after[k] - before[k] for k in KINDS}


def test_free_device_memory_does_not_drift(amd):
    """Five create / three host jobs / destroy cycles; free device memory after every cycle, as the runtime reports it."""
    import torch
    host = [frames(amd, 640, 360, 4, 4 * b, device=False) for b in range(3)]
    before = counts(amd)
    free = []
    for cycle in range(5):
        c = fresh_context(amd)
        try:
            host_jobs(amd, c, host)
        finally:
            c.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    drift = [free[k - 1] - free[k] for k in range(2, 5)]  # bytes lost from one cycle to the next over cycles 2 .. 5
    print("free device memory after each cycle:", free, "lost per cycle from the second on:", drift)
    assert max(drift) <= PARENT_MAX_DRIFT_BYTES, (free, drift)
    if before is not None:
        assert counts(amd) == before
