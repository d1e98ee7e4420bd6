"""akz_resection_seeded_problems on the GPU: every problem of a call equals akz_resection_seeded_host on it with stream
stream_base + p, bit for bit -- the kept indices, every word of the pose, the accepted fits and trials_run -- and nothing is
written beyond a problem's kept count or by a refused call.  The scenes are those of tests/resection_numpy.py with 0.5 px of
noise, judged at 2 px, so that the refit has sets to grow; every problem has a camera of its own."""
import ctypes as C

import numpy as np
import pytest

import resection_numpy as rn

pytestmark = pytest.mark.gpu

SIZES = (5, 6, 7, 255, 256, 257, 1000)   # below K, K, the 256-lane boundaries, several strides
BASE = 5                                 # stream_base
EPS = 2.0
FILL = 0xA5A5A5A5


def camera(s):
    return (1400.0 + 3 * s, 1400.0 - 2 * s, 960.0 + 1.5 * s, 540.0 - s)


def scene(seed, n, s, outliers=0.2):
    n_out = int(n * outliers) if n > 7 else 0
    sc = rn.make_scene(seed, n - n_out, n_out, noise=0.5 if n > 7 else 0.0, camera=camera(s))
    return sc["points"], sc["pixels"], sc["camera"]


@pytest.fixture(scope="module")
def problems():
    """0 .. 6: scenes of SIZES; 7: empty; 8: 100 coplanar points (no trial has a model); 9: 100 outliers and nothing else; 10:
    problem 5 again; 11: problem 3 mirrored through the camera centre -- the same pixels from points that are all behind it.
    (built once, left unchanged)"""
    pr = [scene(300 + i, n, i) for i, n in enumerate(SIZES)]
    pr.append((np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), camera(7)))
    sc = rn.make_scene(308, 100, 0, camera=camera(8))
    xc = sc["points"].astype(np.float64) @ sc["R"].T + sc["t"]
    xc[:, 2] = 5.0
    flat = ((xc - sc["t"]) @ sc["R"]).astype(np.float32)
    pr.append((flat, rn.project(sc["R"], sc["t"], flat, camera(8))[0].astype(np.float32), camera(8)))
    sc = rn.make_scene(309, 0, 100, camera=camera(9))
    pr.append((sc["points"], sc["pixels"], camera(9)))
    pr.append(pr[5])
    sc = rn.make_scene(303, 204, 51, noise=0.5, camera=camera(3))
    xc = sc["points"].astype(np.float64) @ sc["R"].T + sc["t"]
    pr.append((((-xc - sc["t"]) @ sc["R"]).astype(np.float32), sc["pixels"], camera(3)))
    return pr


def options(amd, max_trials=200, confidence=0.0, its=0, **kw):
    kw.setdefault("stream_base", BASE)
    return amd.RansacOptions(model_kind=amd.RANSAC_RESECTION, max_trials=max_trials, confidence=confidence, refine_iterations=its,
                             epsilon_inliers=EPS, **kw)


def host(amd, problems, opt):
    return [amd.resection_seeded_host(*q, opt, stream=opt.stream_base + p) for p, q in enumerate(problems)]


def same(got, exp, what):
    assert len(got) == len(exp), what
    for p, ((gk, gp, gi, gt), (ek, ep, ei, et)) in enumerate(zip(got, exp)):
        assert gk.dtype == np.uint32 and np.array_equal(gk, ek), (what, p, len(gk), len(ek))
        assert np.array_equal(gp.words(), ep.words()), (what, p, gp.words(), ep.words())
        assert (gi, gt) == (ei, et), (what, p, gi, ei, gt, et)


@pytest.mark.parametrize("max_trials", [200, 128])
@pytest.mark.parametrize("confidence", [0.0, 0.99])
@pytest.mark.parametrize("its", [0, 2])
def test_twelve_problems_equal_the_host_statement(ctx, amd, problems, max_trials, confidence, its):
    opt = options(amd, max_trials, confidence, its)
    exp = host(amd, problems, opt)
    same(ctx.resection_seeded(problems, opt), exp, (max_trials, confidence, its))
    # what the cases are there for
    found = [e[1].found for e in exp]
    assert found == [0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0], found
    assert [e[3] for e in exp][:2] == [0, 128 if confidence else max_trials] and exp[7][3] == 0
    assert exp[8][3] == exp[9][3] == exp[11][3] == max_trials        # no winner: the rule never stops them
    assert all(len(e[0]) == 0 and not e[1].words().any() and e[2] == 0 for e, f in zip(exp, found) if not f)
    if confidence and max_trials == 200:   # both stopping branches: four scenes stop after the first round, two run to the end
        assert [e[3] for e in exp][1:7] == [128, 128, 128, 200, 200, 128]
    if its:
        assert any(e[2] > 0 for e in exp)


@pytest.mark.parametrize("max_trials", [1025, 2177])   # one trial past a window of eight rounds, and past two windows
@pytest.mark.parametrize("confidence", [0.0, 0.99])
def test_past_a_window_of_rounds(ctx, amd, problems, max_trials, confidence):
    """The rounds driver's window path, which 200 trials never reach: after eight rounds the host reads the count of problems still
    running and uploads the next window's need table.  With the stopping rule one call holds problems that cross the window (the
    outliers and the plane have no winner, so the rule never stops them) and scenes that finished before it."""
    sub = [problems[p] for p in (2, 4, 5, 8, 9)]   # 7, 256 and 257 correspondences, the plane, the outliers
    opt = options(amd, max_trials, confidence, 2)
    exp = host(amd, sub, opt)
    same(ctx.resection_seeded(sub, opt), exp, (max_trials, confidence))
    trials = [e[3] for e in exp]
    if confidence:
        assert trials[4] == max_trials and any(t < 1024 for t in trials[:3]), trials
    else:
        assert trials == [max_trials] * 5, trials


def test_nothing_written_beyond_the_counts_or_by_a_refused_call(ctx, amd, problems):
    L = amd.lib()
    opt = options(amd, 200, 0.0, 2)
    exp = host(amd, problems, opt)

    def filled():
        a = amd._ResectionArgs(problems)
        a.kept[:] = FILL
        a.n_kept[:] = FILL
        a.its[:] = FILL
        a.trials[:] = FILL
        C.memset(a.poses, 0xA5, C.sizeof(a.poses))
        return a

    def untouched(a):
        return (np.all(a.kept == FILL) and np.all(a.n_kept == FILL) and np.all(a.its == FILL) and np.all(a.trials == FILL)
                and bytes(a.poses) == b"\xa5" * C.sizeof(a.poses))

    a = filled()
    assert L.akz_resection_seeded_problems(ctx._h, a.problems, len(a.sizes), C.byref(opt), *a.tail()) == 0
    same(a.results(), exp, "filled")
    off = 0
    for p, n in enumerate(a.sizes):
        assert np.all(a.kept[off + int(a.n_kept[p]):off + n] == FILL), p
        off += n
    bad_cam = list(problems)
    bad_cam[4] = (bad_cam[4][0], bad_cam[4][1], (0.0, 1400.0, 960.0, 540.0))
    for pr, o in ((problems, opt.copy(model_kind=1)), (problems, opt.copy(model_kind=3)), (problems, opt.copy(guided=1)),
                  (problems, opt.copy(confidence=1.0)), (problems, opt.copy(max_trials=(1 << 24) + 1)),
                  (problems, opt.copy(epsilon_inliers=float("nan"))), (bad_cam, opt)):
        a = filled()
        a2 = amd._ResectionArgs(pr)
        assert L.akz_resection_seeded_problems(ctx._h, a2.problems, len(a2.sizes), C.byref(o), *a.tail()) != 0
        assert untouched(a)
    a = filled()
    a.problems[6].points = None
    assert L.akz_resection_seeded_problems(ctx._h, a.problems, len(a.sizes), C.byref(opt), *a.tail()) != 0 and untouched(a)
    a = filled()
    assert L.akz_resection_seeded_problems(None, a.problems, len(a.sizes), C.byref(opt), *a.tail()) != 0 and untouched(a)
    assert L.akz_resection_seeded_problems(ctx._h, a.problems, 0, C.byref(opt), *a.tail()) == 0 and untouched(a)


def test_one_problem_and_forty(ctx, amd, problems):
    """one problem: 8 workgroups with helper waves; forty: 320 workgroups... and 70 problems, 560 workgroups, the plain form"""
    opt = options(amd, 200, 0.99, 2)
    same(ctx.resection_seeded(problems[6:7], opt), host(amd, problems[6:7], opt), "one")
    many = [problems[p % 7] for p in range(40)]
    exp = host(amd, many, opt)
    same(ctx.resection_seeded(many, opt), exp, "forty")
    assert any(not np.array_equal(exp[p][1].words(), exp[p + 7][1].words()) for p in range(1, 7))   # (streams differ)
    more = [problems[1 + p % 6] for p in range(70)]
    same(ctx.resection_seeded(more, opt), host(amd, more, opt), "seventy")


def test_batch_equals_the_loop_and_scratch_is_reused(ctx, amd, problems):
    opt = options(amd, 200, 0.0, 2)
    batch = ctx.resection_seeded(problems, opt)          # (after the larger calls of the test above, on the same context)
    before = amd.debug_resource_counts()
    loop = [ctx.resection_seeded([q], opt.copy(stream_base=BASE + p))[0] for p, q in enumerate(problems)]
    same(loop, batch, "loop")
    same(ctx.resection_seeded(problems, opt), batch, "again")
    after = amd.debug_resource_counts()
    assert (after["device_blocks"], after["device_bytes"], after["pinned_bytes"]) == (before["device_blocks"], before["device_bytes"],
                                                                                     before["pinned_bytes"])
