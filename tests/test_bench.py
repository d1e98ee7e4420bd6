"""bench.py without a GPU: what a plain run times against --full, and the arrays --dump-outputs writes."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("size", "<f4"),
                     ("octave", "<u8"), ("class_id", "<u8"), ("angle", "<f4"), ("_pad", "<u4")])


def test_plain_run_times_exactly_the_steps_asked_for():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.regions, a.full, a.dump_outputs) == (7, 2, 1, False, None)
    f = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full"])
    assert (f.steps, f.regions, f.full) == (7, 5, True)
    assert bench.parse_args(["--full", "--regions", "2"]).regions == 2
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"


class _Result:
    """The two accessors of akaze_amd.Result that step_outputs reads."""

    def __init__(self, per_image):
        self._imgs = per_image

    def keypoints(self, i):
        return self._imgs[i][0]

    def descriptors(self, i):
        return self._imgs[i][1]


def _image(rng, n):
    kp = np.zeros(n, KP_DTYPE)
    for c in ("x", "y", "response", "size", "angle"):
        kp[c] = rng.random(n, dtype=np.float32) * 100
    kp["octave"] = rng.integers(0, 4, n)
    kp["class_id"] = rng.integers(0, 9, n)
    return kp, rng.integers(0, 256, (n, 61), dtype=np.uint8)


def test_step_outputs_are_the_frames_in_order(tmp_path):
    rng = np.random.default_rng(1)
    imgs = [_image(rng, n) for n in (5, 0, 7, 3)]
    results = [_Result(imgs[:2]), _Result(imgs[2:])]   # two batches of a step: frames 0-1 and 2-3
    outs = bench.step_outputs(results, [0, 2, 4], 4)
    assert sorted(outs) == ["descriptors", "keypoints", "keypoints_per_frame"]
    assert outs["keypoints_per_frame"].tolist() == [5, 0, 7, 3]
    kp = np.concatenate([k for k, _ in imgs])
    for j, c in enumerate(bench.KEYPOINT_COLUMNS):
        assert np.array_equal(outs["keypoints"][:, j], kp[c].astype(np.float64)), c
    assert np.array_equal(outs["descriptors"], np.concatenate([d for _, d in imgs]).astype(np.float32))
    bench.write_outputs(str(tmp_path), outs)
    for name, a in outs.items():
        b = np.load(tmp_path / f"{name}.npy")
        assert b.dtype in (np.float32, np.float64) and np.array_equal(a, b)


def test_step_outputs_sample_a_large_step_the_same_way_every_time(monkeypatch):
    rng = np.random.default_rng(2)
    imgs = [_image(rng, 400) for _ in range(3)]
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", (1 << 16) + 300 * 300)   # room for about 300 of the 1200 rows
    a = bench.step_outputs([_Result(imgs)], [0, 3], 3)
    b = bench.step_outputs([_Result(imgs)], [0, 3], 3)
    rows = a["sample_rows"].astype(np.int64)
    assert 0 < len(rows) < 1200 and np.all(np.diff(rows) > 0)
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_MAX_BYTES - (1 << 16)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    kp = np.concatenate([k for k, _ in imgs])
    assert np.array_equal(a["keypoints"][:, 0], kp["x"][rows].astype(np.float64))
    assert np.array_equal(a["descriptors"], np.concatenate([d for _, d in imgs])[rows].astype(np.float32))
    assert a["keypoints_per_frame"].tolist() == [400, 400, 400]


def test_dump_outputs_is_refused_with_the_stub_context(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--dump-outputs", str(tmp_path / "d")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--dump-outputs" in p.stderr
    assert not (tmp_path / "d").exists()
