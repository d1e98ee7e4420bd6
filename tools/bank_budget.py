#!/usr/bin/env python3
"""The feature bank under a keypoint budget (akz_bank_create_from_results_budget, k_bank_select) against the flow it replaces.

    timeout -k 10 900 python tools/bank_budget.py [--regions 5] [--calls 20] [--baseline OTHER/akaze-rust_amd] [--out FILE]

Workloads and settings are those of tools/feature_bank.py: synth_frame features of one scene with shifts at 1920x1080, kept as
extraction results -- 1 pair over 2 sets, the 56 ordered pairs of 8 sets, 240 pairs (i, i + 1) over 240 sets --, the normalised
fundamental matrix (model_kind 3) at 2 px with two refit iterations, 1 000 trials, ratio 0.86, confidence 0.99.  The budget: at most
1 000 keypoints per set, SPREAD mode, robust 0.9.  Every figure is the median of --regions regions of --calls synchronous calls each,
per call, with the least and the greatest region:
  (a) `flow`         what the budgeted bank replaces, on THIS build: keypoints() / descriptors() of every image, keypoint_budget_sets,
                     a numpy slice per set, feature_bank(host sets), close;
      `parent_flow`  with --baseline: the same on the build under that directory, in a child process of its own before this process
                     opens the GPU (the leg the feature is held against);
  (b) `budget_bank`  feature_bank(results, budget=...) and close;
  (c) `plain_bank`   feature_bank(results) and close: (b) minus (c) is what the budget itself costs;
  (d) `select_ms`    k_bank_select between two events (akz_debug_kernel_rows, profiling on; the launch alone), against `gather_ms`,
                     k_bank_gather over as many rows through akz_debug_bank_gather, and `d2d_ms`, a device-to-device copy of the same
                     bytes between two events;
  (e) `pairs_budget` the bank pairs call over the budgeted bank against `pairs_full`, the same call over the full bank.
`equal`: the budgeted bank holds the bytes of the bank made from the host flow's sliced sets.  Prints one JSON document (and writes
it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "akaze-rust_amd")
if "--pkg" in sys.argv:  # the child of --baseline: the build under PKG (its library and its binding), set before the import
    PKG = os.path.abspath(sys.argv[sys.argv.index("--pkg") + 1])
    os.environ["AKAZE_HIP_LIB"] = os.path.join(PKG, "libakaze_hip.so")
sys.path.insert(0, os.path.join(PKG, "python"))
import akaze_amd as A  # noqa: E402

TRIALS, RATIO, EPS, FITS, CONFIDENCE = 1000, 0.86, 2.0, 2, 0.99
MAX_KEYPOINTS, ROBUST = 1000, 0.9
WORKLOADS = [("1 pair over 2 sets", 2, [(0, 1)]),
             ("56 pairs over 8 sets", 8, [(a, b) for a in range(8) for b in range(8) if a != b]),
             ("240 pairs over 240 sets", 240, [(i, (i + 1) % 240) for i in range(240)])]


def options():
    return A.RansacOptions(model_kind=A.RANSAC_FUNDAMENTAL_NORMALISED, lowes_ratio=RATIO, max_trials=TRIALS, epsilon_inliers=EPS,
                           confidence=CONFIDENCE, refine_iterations=FITS)


def extract(ctx, n_sets, idx=31):
    """results whose images are the sets, in order: batches of up to 8 frames, frame i shifted by (5, 3) x (i mod 16)"""
    import torch
    out = []
    for first in range(0, n_sets, 8):
        fr = [A.synth_frame(1920, 1080, idx, shift=(5 * (i % 16), 3 * (i % 16))) for i in range(first, min(first + 8, n_sets))]
        out.append(ctx.extract_features(torch.from_numpy(np.stack(fr)).cuda(), keep_all_planes=False))
    return out


def host_sliced(ctx, results):
    """the host flow up to the sliced sets"""
    feats = [(r.keypoints(i), r.descriptors(i)) for r in results for i in range(r.num_images)]
    cut = ctx.keypoint_budget_sets(feats, MAX_KEYPOINTS, A.BUDGET_SPREAD, ROBUST)
    return [(np.ascontiguousarray(k[i]), np.ascontiguousarray(d[i])) for (k, d), (i, _) in zip(feats, cut)]


def host_flow(ctx, results):
    ctx.feature_bank(host_sliced(ctx, results)).close()


def regions(fn, n_regions, calls):
    fn()
    per_call = []
    for _ in range(n_regions):
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        per_call.append((time.perf_counter() - t) * 1e3 / calls)
    return {"ms": round(statistics.median(per_call), 4), "min_max": [round(min(per_call), 4), round(max(per_call), 4)]}


def parent_rows(n_regions, calls):
    """(child) the host flow on the build under --pkg, which has no budgeted bank"""
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    rows = []
    for name, n_sets, _ in WORKLOADS:
        results = extract(ctx, n_sets)
        rows.append({"workload": name, **regions(lambda: host_flow(ctx, results), n_regions, calls)})
        for r in results:
            r.close()
    ctx.close()
    return rows


def event_ms(fn, n):
    import torch
    got = []
    for _ in range(n + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        got.append(a.elapsed_time(b))
    return round(statistics.median(got[1:]), 4)


def kernel_ms(ctx, fn, kernel, n):
    """the median span of `kernel`'s one launch per call of fn, from the context's kernel rows"""
    ctx.set_profiling(1)
    ctx.kernel_rows(reset=True)
    got = []
    for _ in range(n):
        fn()
        rows = [r for r in ctx.kernel_rows(reset=True) if r["kernel"] == kernel]
        assert len(rows) == 1 and rows[0]["launches"] == 1, rows
        got.append(rows[0]["ms"])
    ctx.set_profiling(0)
    return round(statistics.median(got), 4)


def workload(ctx, name, n_sets, pairs, n_regions, calls):
    import torch
    opt = options()
    budget = A.KeypointBudget(MAX_KEYPOINTS, A.BUDGET_SPREAD, ROBUST)
    results = extract(ctx, n_sets)
    full = ctx.feature_bank(results)
    cut = ctx.feature_bank(results, budget=budget)
    kept, rows = cut.info()["rows"], full.info()["rows"]
    row = {"workload": name, "sets": n_sets, "pairs": len(pairs), "rows": rows, "rows_per_set": round(rows / n_sets, 1), "kept_rows": kept,
           "max_keypoints": MAX_KEYPOINTS, "mode": "AKZ_BUDGET_SPREAD", "robust": ROBUST, "regions": n_regions, "calls_per_region": calls}
    reference = ctx.feature_bank(host_sliced(ctx, results))
    row["equal"] = all(a.tobytes() == b.tobytes() for a, b in zip(cut.download(), reference.download())) and cut.info() == reference.info()
    reference.close()
    feats = [(r.keypoints(i), r.descriptors(i)) for r in results for i in range(r.num_images)]
    legs = {"flow": lambda: host_flow(ctx, results),
            "budget_bank": lambda: ctx.feature_bank(results, budget=budget).close(),
            "plain_bank": lambda: ctx.feature_bank(results).close(),
            "budget_bank_from_sets": lambda: ctx.feature_bank(feats, budget=budget).close(),
            "pairs_budget": lambda: ctx.match_features_seeded_pairs(cut, pairs, opt),
            "pairs_full": lambda: ctx.match_features_seeded_pairs(full, pairs, opt)}
    for leg, fn in legs.items():
        row[leg] = regions(fn, n_regions, calls)
    # the launch alone, against the plain gather over as many rows and a device-to-device copy of the same bytes
    n = n_regions * calls
    row["select_ms"] = kernel_ms(ctx, legs["budget_bank"], "k_bank_select", n)
    src = torch.randint(0, 255, (max(kept, 1), 64), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    row["gather_ms"] = kernel_ms(ctx, lambda: ctx.debug_bank_gather(src, 61, dst), "k_bank_gather", n)
    row["d2d_ms"] = event_ms(lambda: dst.copy_(src), n)
    row["select_over_gather"] = round(row["select_ms"] / row["gather_ms"], 3) if row["gather_ms"] > 0 else None
    row["select_over_d2d"] = round(row["select_ms"] / row["d2d_ms"], 3) if row["d2d_ms"] > 0 else None
    row["budget_bank_over_flow"] = round(row["budget_bank"]["ms"] / row["flow"]["ms"], 3)
    row["budget_cost_ms"] = round(row["budget_bank"]["ms"] - row["plain_bank"]["ms"], 4)
    row["pairs_budget_over_pairs_full"] = round(row["pairs_budget"]["ms"] / row["pairs_full"]["ms"], 3)
    full.close()
    cut.close()
    for r in results:
        r.close()
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--baseline", help="akaze-rust_amd directory of the parent build: its host flow is the `parent_flow` leg")
    ap.add_argument("--pkg", help="(child) the akaze-rust_amd directory of the build to measure")
    ap.add_argument("--rows", action="store_true", help="(child) print the parent leg's rows alone")
    args = ap.parse_args()
    if args.rows:
        print(json.dumps(parent_rows(args.regions, args.calls)))
        return
    parent = None
    if args.baseline:  # (before this process opens the GPU)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", os.path.abspath(args.baseline), "--regions", str(args.regions),
                              "--calls", str(args.calls), "--rows"], check=True, stdout=subprocess.PIPE, timeout=420).stdout
        parent = json.loads(out)
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    rows = [workload(ctx, name, n_sets, pairs, args.regions, args.calls) for name, n_sets, pairs in WORKLOADS]
    if parent:
        for row, par in zip(rows, parent):
            assert row["workload"] == par["workload"]
            row["parent_flow"] = {"ms": par["ms"], "min_max": par["min_max"]}
            row["budget_bank_over_parent_flow"] = round(row["budget_bank"]["ms"] / par["ms"], 3)
            row["budget_bank_slower_than_parent_flow"] = bool(row["budget_bank"]["ms"] > par["ms"])
    doc = {"tool": "tools/bank_budget.py", "device": torch.cuda.get_device_name(0), "trials": TRIALS, "ratio": RATIO, "epsilon_px": EPS,
           "refine_iterations": FITS, "confidence": CONFIDENCE, "model_kind": "AKZ_RANSAC_FUNDAMENTAL_NORMALISED", "workloads": rows}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
