#!/usr/bin/env python3
"""The forms a job of extract_features can take, one pass: a lone 640x480 frame through the synchronous call, the same frame
begun and finished (batch path, march gate lowered to the job's size), 12 x 1280x720 begun with input_ready (automatic
preparation, resident tail, level 0 running ahead), a lone 1920x1080 synchronous call, and the two per-op calls gaussian_blur and
detector_response on a 640x480 plane.
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- python tools/job_forms.py --trace
    python tools/job_forms.py --compare DIR_A DIR_B     (two such traces: same GPU work?  prints one JSON line)
--trace runs without the placement probe (akz_debug_set_schedule key 2), whose stream replacements depend on timing: the
streams are then the same from run to run.  AKAZE_HIP_LIB picks the library (akaze_amd.LIB_PATH)."""
import collections
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "akaze-rust_amd", "python"))


def one_pass():
    import numpy as np
    import torch
    import akaze_amd as A
    small = torch.from_numpy(A.synth_frame(640, 480, 7)[None]).cuda()
    batch = torch.from_numpy(np.stack([A.synth_frame(1280, 720, 20 + i) for i in range(12)])).cuda()
    hd = torch.from_numpy(A.synth_frame(1920, 1080, 3)[None]).cuda()
    plane = torch.from_numpy(np.random.default_rng(31).uniform(0, 1, (480, 640)).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.debug_set_schedule(2, 1)
    counts = []
    for name, run in (("sync_640x480", lambda: ctx.extract_features(small, keep_all_planes=False)),
                      ("begun_640x480", lambda: ctx.extract_begin(small, keep_all_planes=False).finish()),
                      ("begun_ready_12x1280x720", lambda: ctx.extract_begin(batch, keep_all_planes=False, input_ready=True).finish()),
                      ("sync_1920x1080", lambda: ctx.extract_features(hd, keep_all_planes=False))):
        res = run()
        ctx.synchronize()
        counts.append((name, [len(res.keypoints(i)) for i in range(res.num_images)]))
        res.close()
    ctx.gaussian_blur(plane, 1.6)
    ctx.detector_response(plane, 2)
    ctx.synchronize()
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps(dict(jobs=counts)))


def read_trace(d, what):
    rows = []
    for p in sorted(glob.glob(os.path.join(d, "**", f"*{what}.csv"), recursive=True)):
        with open(p, newline="") as f:
            rows += list(csv.DictReader(f))
    return rows


def by_lane(rows, name_key):
    """{lane: [names in start order]} with lanes numbered by first appearance; a lane is a stream where the trace has them"""
    key = next((k for k in ("Stream_Id", "Queue_Id") if rows and k in rows[0]), None)
    rows = sorted(rows, key=lambda r: int(r["Start_Timestamp"]))
    lanes, order = collections.OrderedDict(), {}
    for r in rows:
        lane = order.setdefault(r[key] if key else "all", len(order))
        lanes.setdefault(lane, []).append(r[name_key])
    return key or "none", lanes


def first_difference(la, lb):
    for lane in sorted(set(la) | set(lb)):
        x, y = la.get(lane, []), lb.get(lane, [])
        if x != y:
            i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            return dict(lane=lane, at=i, a=x[i:i + 3], b=y[i:i + 3], lengths=[len(x), len(y)])
    return None


def compare(a, b):
    out = {}
    for what, trace, name_key in (("kernels", "kernel_trace", "Kernel_Name"), ("copies", "memory_copy_trace", "Direction")):
        # (which engine ran a copy -- SDMA or a blit kernel -- is the runtime's choice: direction and order are what is compared)
        ra, rb = read_trace(a, trace), read_trace(b, trace)
        key, la = by_lane(ra, name_key)
        _, lb = by_lane(rb, name_key)
        na, nb = collections.Counter(r[name_key] for r in ra), collections.Counter(r[name_key] for r in rb)
        out[what] = dict(lanes_are=key, count=[len(ra), len(rb)], lanes=[len(la), len(lb)], same_names_with_counts=na == nb,
                         same_sequence_per_lane=la == lb)
        if na != nb:
            out[what]["count_differences"] = {k: [na[k], nb[k]] for k in sorted(set(na) | set(nb)) if na[k] != nb[k]}
        if la != lb:
            out[what]["first_difference"] = first_difference(la, lb)
    out["same_gpu_work"] = out["kernels"]["count"][0] > 0 and all(out[w]["same_names_with_counts"] and out[w]["same_sequence_per_lane"]
                                                                  for w in ("kernels", "copies"))
    print(json.dumps(out))
    return 0 if out["same_gpu_work"] else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["--trace"]:
        one_pass()
    elif sys.argv[1:2] == ["--compare"] and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
