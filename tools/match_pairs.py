#!/usr/bin/env python3
"""akz_match_features_pairs against a loop of akz_match_features over the same pairs.

    timeout -k 10 900 python tools/match_pairs.py [--reps 5] [--out FILE]                   # timings (one GPU process)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/match_pairs.py --trace   # kernel stats

Workloads, from synth_frame features of one scene with shifts (the frames overlap, so every pair verifies): exhaustive
ordered pairs of 8 and 16 frames at 1920x1080, consecutive pairs of 32 frames at 1920x1080, a few 3840x2160 pairs, and a
lone 1080p pair; all at 1 000 trials, epsilon 3.0, ratio 0.86.  Per workload the loop and the batch alternate rep by rep
(medians of --reps after one warm-up, each rep reseeded: both consume the same random stream) and report pairs/s; the
batch's split (akz_debug_match_pairs_split: uploads, scans, host draws, trials, pick + filter, read-back) is the median of
timed runs of their own.  Prints one JSON document (and writes it to --out if given).  --trace: one pass of every call."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akaze-rust_amd", "python"))
import akaze_amd as A  # noqa: E402

TRIALS, EPS, RATIO = 1000, 3.0, 0.86
SPLIT = ["uploads", "scans", "host_draws", "trials", "pick_filter", "readback"]


def features(ctx, w, h, n, idx=31):
    out = []
    for i in range(n):
        r = ctx.extract_features(A.synth_frame(w, h, idx, shift=(5 * i, 3 * i)), keep_all_planes=False)
        out.append((r.keypoints(), r.descriptors()))
    return out


def loop(ctx, feats, pairs):
    return [A.match_features(feats[a][0], feats[a][1], feats[b][0], feats[b][1], RATIO, TRIALS, EPS, ctx=ctx) for a, b in pairs]


def batch(ctx, feats, pairs):
    return ctx.match_features_pairs(feats, pairs, RATIO, TRIALS, EPS)


def timed(fn):
    A.random_seed(42, 69)
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def workload(ctx, name, feats, pairs, reps):
    A.random_seed(42, 69)
    a = loop(ctx, feats, pairs)
    A.random_seed(42, 69)
    b = batch(ctx, feats, pairs)
    same = all(np.array_equal(x, y) for x, y in zip(a, b))
    t = {"loop": [], "batch": []}
    for _ in range(reps):
        t["loop"].append(timed(lambda: loop(ctx, feats, pairs)))
        t["batch"].append(timed(lambda: batch(ctx, feats, pairs)))
    split = []
    A.lib().akz_debug_match_pairs_split(ctx._h, 1, None)
    ms = (C.c_double * 6)()
    for _ in range(reps):
        timed(lambda: batch(ctx, feats, pairs))
        A.lib().akz_debug_match_pairs_split(ctx._h, 1, ms)
        split.append(list(ms))
    A.lib().akz_debug_match_pairs_split(ctx._h, 0, None)
    med = {k: statistics.median(v) for k, v in t.items()}
    raw = [len(ctx.descriptor_match(feats[x][1], feats[y][1], 10000, RATIO)) for x, y in pairs]
    row = {
        "workload": name, "pairs": len(pairs), "matches_per_pair_median": statistics.median(raw),
        "pairs_drawing": sum(r >= 8 for r in raw), "keypoints_per_set_median": statistics.median(len(f[0]) for f in feats),
        "identical_to_loop": same,
        "loop_ms": round(med["loop"], 3), "batch_ms": round(med["batch"], 3),
        "loop_ms_min_max": [round(min(t["loop"]), 3), round(max(t["loop"]), 3)],
        "batch_ms_min_max": [round(min(t["batch"]), 3), round(max(t["batch"]), 3)],
        "loop_pairs_per_s": round(len(pairs) / med["loop"] * 1e3, 1),
        "batch_pairs_per_s": round(len(pairs) / med["batch"] * 1e3, 1),
        "speedup": round(med["loop"] / med["batch"], 2),
        "batch_split_ms": {k: round(statistics.median(s[i] for s in split), 3) for i, k in enumerate(SPLIT)},
        "runs": reps,
    }
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    f1080 = features(ctx, 1920, 1080, 32)
    f4k = features(ctx, 3840, 2160, 3)
    jobs = [
        ("1 pair 1080p", f1080[:2], [(0, 1)]),
        ("exhaustive 8 x 1080p", f1080[:8], [(a, b) for a in range(8) for b in range(8) if a != b]),
        ("exhaustive 16 x 1080p", f1080[:16], [(a, b) for a in range(16) for b in range(16) if a != b]),
        ("consecutive 32 x 1080p", f1080, [(i, i + 1) for i in range(31)]),
        ("4K pairs", f4k, [(0, 1), (1, 2), (0, 2), (2, 0)]),
    ]
    if args.trace:
        for _, feats, pairs in jobs:
            loop(ctx, feats, pairs)
            batch(ctx, feats, pairs)
        torch.cuda.synchronize()
        return
    rows = [workload(ctx, name, feats, pairs, args.reps) for name, feats, pairs in jobs]
    doc = {"tool": "tools/match_pairs.py", "device": torch.cuda.get_device_name(0), "trials": TRIALS, "epsilon": EPS,
           "ratio": RATIO, "workloads": rows}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
