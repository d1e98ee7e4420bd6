"""A job's launches depend on the job and on the context's settings, not on what the context ran before.

Three jobs that take three different forms of the begin half -- the lone path, the batch path with the march gate lowered to the
job's size, the batch path with automatic preparation (marches, resident tail, level 0 running ahead) -- are recorded alone on
a fresh context each, then in one sequence on one context in two orders, with per-op calls in between (in the second order:
between a job's begin and its finish).  The kernel rows of the begin half and the results must be those of the job alone.

What is compared of akz_debug_kernel_rows: the rows of the begin half's kernels (kinds 1 .. 5), everything but their time.
The candidate sort's rows (the finish half) carry the capacity of the job's candidate list, which follows the candidate
count of the job before by design (extract_begin: cand_cap_hint, last_cand_shape): they are left out."""
import hashlib

import numpy as np
import pytest

from test_gpu_ops import detector_expected, dev, host, rand_img, same

pytestmark = pytest.mark.gpu

JOBS = ["sync_640x480", "begun_640x480", "begun_ready_12x1280x720"]
ORDERS = [[0, 1, 2], [2, 1, 0, 1]]  # (the second: largest first, and the begun small job on either side of the synchronous one)

FORCED = {
    "default": lambda c: None,
    "marches_forced": lambda c: (c.set_prep_mode(3), c.set_detector_mode(5)),
    "tiled_forced": lambda c: (c.set_prep_mode(0), c.set_detector_mode(0)),
    # every preparation a launch of its own: small jobs then stay in the automatic mode, and the blur and the contrast passes of
    # the begun 640x480 job see the lowered march gate as well
    "own_preparation": lambda c: c.debug_set_schedule(6, 1),
}

FLOAT_FIELDS = ("x", "y", "response", "size", "angle")


def digest(keypoints, descriptors, contrast):
    """keypoints (by field: the padding is nobody's), descriptors and contrast factor of every image"""
    h = hashlib.sha256()
    for kp, d, k in zip(keypoints, descriptors, contrast):
        for f in FLOAT_FIELDS:
            h.update(np.ascontiguousarray(kp[f] + np.float32(0)).tobytes())  # (-0.0 == +0.0)
        for f in ("octave", "class_id"):
            h.update(np.ascontiguousarray(kp[f]).tobytes())
        h.update(np.ascontiguousarray(d).tobytes())
        h.update(np.float64(k).tobytes())
    return h.hexdigest()


def begin_rows(rows):
    return [(r["kernel"], r["kind"], r["param"], r["w"], r["h"], r["n"], r["launches"], r["px"], r["px_steps"])
            for r in rows if 1 <= r["kind"] <= 5]


@pytest.fixture(scope="module")
def inputs(amd, ref):
    import torch
    small = amd.synth_frame(640, 480, 7)
    batch = np.stack([amd.synth_frame(1280, 720, 20 + i) for i in range(12)])
    plane = rand_img(480, 640, seed=31)
    rf = ref.extract(small)
    want = dict(small_digest=digest([rf.keypoints()], [rf.descriptors()], [rf.contrast]), n_small=len(rf.keypoints()),
                blur=ref.gaussian_blur(plane, 1.6), det=detector_expected(ref, plane, 2))
    rf.close()
    d = dict(small=torch.from_numpy(small[None]).cuda(), batch=torch.from_numpy(batch).cuda(), plane=dev(plane))
    torch.cuda.synchronize()
    return d, want


def begin_job(c, job, d):
    if job == 0:
        return c.extract_features(d["small"], keep_all_planes=False)
    if job == 1:
        return c.extract_begin(d["small"], keep_all_planes=False)
    return c.extract_begin(d["batch"], keep_all_planes=False, input_ready=True)


def record(c, job, d, between=None):
    """(begin rows, digest) of one job; `between`: called between the job's begin and its finish"""
    res = begin_job(c, job, d)
    if between and job != 0:
        between()
    if job != 0:
        res = res.finish()
    c.synchronize()
    rows = begin_rows(c.kernel_rows(reset=True))
    n = res.num_images
    dig = digest([res.keypoints(i) for i in range(n)], [res.descriptors(i) for i in range(n)], [res.contrast(i) for i in range(n)])
    res.close()
    return rows, dig


def per_op_calls(c, d, want):
    """outside a job: the context's stream, the mode as set, the 8 Mpx march gate -- against the oracle, as tests/test_gpu_ops.py"""
    same(host(c.gaussian_blur(d["plane"], 1.6)), want["blur"])
    got = c.detector_response(d["plane"], 2)
    for name, exp in want["det"].items():
        same(host(got[name]), exp)


def fresh(amd, force):
    import torch
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    c.set_profiling(1)  # (level 1 keeps the fork)
    force(c)
    return c


@pytest.mark.parametrize("forced", list(FORCED), ids=list(FORCED))
def test_a_jobs_form_does_not_depend_on_the_jobs_before(amd, inputs, forced):
    d, want = inputs
    alone = []
    for job in range(len(JOBS)):
        c = fresh(amd, FORCED[forced])
        try:
            alone.append(record(c, job, d))
        finally:
            c.close()
    for job, (rows, _) in enumerate(alone):
        assert rows, (forced, JOBS[job], "no rows: profiling is off?")
        print(forced, JOBS[job], rows)
    assert want["n_small"] > 50
    assert alone[0][1] == want["small_digest"], (forced, "the lone frame against the oracle")
    assert alone[1][1] == alone[0][1], (forced, "begin / finish against the synchronous call")
    if forced == "default":
        # two forms of one frame: behind big_px_async the full-resolution detectors march (the gate lowered to the job's size)
        kinds = lambda rows: sorted((r[1], r[2], r[3], r[4]) for r in rows)
        assert kinds(alone[0][0]) != kinds(alone[1][0]), alone[0][0]
        assert any(r[1] == 5 for r in alone[1][0]) and not any(r[1] == 5 for r in alone[0][0])

    c = fresh(amd, FORCED[forced])
    try:
        for k, order in enumerate(ORDERS):
            for job in order:
                if k == 0:
                    per_op_calls(c, d, want)
                    got = record(c, job, d)
                else:
                    got = record(c, job, d, between=lambda: per_op_calls(c, d, want))
                assert got[0] == alone[job][0], (forced, order, JOBS[job], "kernel rows")
                assert got[1] == alone[job][1], (forced, order, JOBS[job], "results")
        per_op_calls(c, d, want)
    finally:
        c.close()
