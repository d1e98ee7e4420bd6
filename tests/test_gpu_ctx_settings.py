"""A context's settings reach its lanes whole, whichever of the setter and akz_ctx_set_lanes is called first.

One 640x360 synthetic frame (the size tests/test_gpu_extract.py deals to lanes: below gates::kLanePx), every stage profiled
(Context.set_profiling(1): level 2 of CtxSettings::profiling, itself one of the settings under test and applied with each row).
Per row of SETTINGS three fresh contexts:
    A  the setting, then set_lanes(2)        B  set_lanes(2), then the setting        C  the setting, no lanes
Each begins two jobs and then finishes them, so that each lane of A and B gets one.  What must agree:
  * akz_debug_kernel_rows (kernel, kind -- which fixes the stage --, param, shape, launches; a context's rows include its lanes'):
    everything between A and B; the begin half's kinds 1 .. 5 between those and C.  The candidate sort's rows (kinds 9 .. 11) are
    left out of the comparison with C: which sort a job takes follows from whether the caller waits for it alone, which no lane's
    job does by design (extract_finish: waited_for), so C's first job sorts in one launch where a lane's takes four.
  * akz_debug_device_libm's last-job value and akz_debug_select_info's mode, between A, B and C.
  * keypoints and descriptor bytes of every job, against a default context's.
Rows whose hook changes no recorded launch of a job this small (prep_mode 0: such a job takes the tiled preparation anyway;
schedule keys 6 and 10: neither the ride of a level's preparation on the diffusion launch before it nor level 0's two-launch
form has a row; key 11 alone: no detector of such a job marches; device_libm alone: its last-job value is 0 wherever the host
selects) agree trivially; the two rows at the end give keys 11 and device_libm something to show: column-march detectors
everywhere, and the selection on the device."""
import pytest

from test_gpu_job_form import digest

pytestmark = pytest.mark.gpu

W, H = 640, 360

SETTINGS = {
    "fed_mode_0": lambda c: c.set_fed_mode(0),
    "prep_mode_0": lambda c: c.set_prep_mode(0),
    "detector_mode_4": lambda c: c.set_detector_mode(4),
    "sched_6": lambda c: c.debug_set_schedule(6, 1),
    "sched_10": lambda c: c.debug_set_schedule(10, 1),
    "sched_11": lambda c: c.debug_set_schedule(11, 1),
    "device_libm_0": lambda c: c.debug_set_device_libm(False),  # (the binding's spelling of mode 0)
    "select_1": lambda c: c.debug_set_select(1),
    "host_sort_1": lambda c: c.debug_set_host_sort(1),
    "march_detectors_sched_11": lambda c: (c.set_detector_mode(5), c.debug_set_schedule(11, 1)),
    "device_select_device_libm_0": lambda c: (c.debug_set_select(2), c.debug_set_device_libm(False)),
}


def run(amd, frame, steps):
    """a fresh context, `steps` applied in order, two jobs -> (all rows, begin-half rows, libm last job, select mode, digests)"""
    import torch
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        for step in steps:
            step(c)
        jobs = [c.extract_begin(frame, keep_all_planes=False) for _ in range(2)]
        res = [j.finish() for j in jobs]
        c.synchronize()
        rows = sorted((r["kernel"], r["kind"], r["param"], r["w"], r["h"], r["n"], r["launches"]) for r in c.kernel_rows(reset=True))
        digests = [digest([r.keypoints(0)], [r.descriptors(0)], [r.contrast(0)]) for r in res]
        for r in res:
            r.close()
        return rows, [r for r in rows if 1 <= r[1] <= 5], c.debug_device_libm()[1], c.debug_select_info()[0], digests
    finally:
        c.close()


@pytest.fixture(scope="module")
def frame_and_default(amd):
    import torch
    frame = torch.from_numpy(amd.synth_frame(W, H, 40)[None]).cuda()
    torch.cuda.synchronize()
    default = run(amd, frame, [lambda c: c.set_profiling(1)])
    assert default[1], "no rows: profiling is off?"
    assert default[4][0] == default[4][1]
    return frame, default


@pytest.mark.parametrize("name", list(SETTINGS), ids=list(SETTINGS))
def test_lanes_run_with_the_contexts_settings_in_either_order(amd, frame_and_default, name):
    frame, default = frame_and_default
    setting = lambda c: (c.set_profiling(1), SETTINGS[name](c))
    lanes = lambda c: c.set_lanes(2)
    a = run(amd, frame, [setting, lanes])
    b = run(amd, frame, [lanes, setting])
    c = run(amd, frame, [setting])
    for label, got in (("A", a), ("B", b), ("C", c)):
        print(name, label, "libm", got[2], "select", got[3], got[0])
    assert a[0] == b[0], (name, "every kernel row, setting first against lanes first")
    assert a[1] == c[1], (name, "begin-half rows, setting then lanes against no lanes")
    assert b[1] == c[1], (name, "begin-half rows, lanes then setting against no lanes")
    assert a[2] == b[2] == c[2], (name, "akz_debug_device_libm: last job", a[2], b[2], c[2])
    assert a[3] == b[3] == c[3], (name, "akz_debug_select_info: mode", a[3], b[3], c[3])
    for label, got in (("A", a), ("B", b), ("C", c)):
        assert got[4] == default[4], (name, label, "keypoints and descriptors against a default context's")
