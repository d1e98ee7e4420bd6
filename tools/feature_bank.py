#!/usr/bin/env python3
"""The feature bank (akz_bank_*) against the flow it replaces: extraction results -> host copies -> akz_match_features_seeded_pairs.

    timeout -k 10 900 python tools/feature_bank.py [--regions 5] [--calls 20] [--baseline OTHER/akaze-rust_amd] [--out FILE]

Workloads: synth_frame features of one scene with shifts at 1920x1080, extracted in batches of up to 8 frames and kept as results --
1 pair over 2 sets, the 56 ordered pairs of 8 sets, and 240 pairs (i, i + 1) over 240 sets --, the normalised fundamental matrix
(model_kind 3) at 2 px with two refit iterations, 1 000 trials, ratio 0.86, confidence 0.99.  Every figure is the median of --regions
regions of --calls synchronous calls each, per call, with the least and the greatest region:
  `flow`        what the bank replaces, on THIS build: keypoints() / descriptors() of every image, then the sets call;
  `parent_flow` with --baseline: the same on the build under that directory, in a child process of its own before this process
                opens the GPU (the sets call is the same code in both builds; this is the leg the feature is held against);
  `sets_call`   the sets call alone over host copies made once (what a caller that keeps its host copies pays per call);
  `bank_flow`   bank creation from the results + the bank call + akz_bank_free;
  `bank_call`   the bank call alone on a bank made once: the re-use case;
  `bank_create` creation from the results + free, and `bank_create_from_sets` from the host copies.
`upload_ms`: the upload interval of akz_debug_match_pairs_split of the sets call (pack on one thread + three copies), median of
--regions x --calls timed calls -- the share of the call the bank removes; the same interval of the bank call is recorded next to it.
`gather_ms`: k_bank_gather between two events (akz_debug_kernel_rows, profiling on; the launch alone, without the table's upload),
against `d2d_ms`, a device-to-device copy of the same bytes between two events.  `equal`: the bank call's outputs are the sets
call's, as bytes.  Prints one JSON document (and writes it to --out)."""
import argparse
import ctypes as C
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


def host_copies(results):
    return [(r.keypoints(i), r.descriptors(i)) for r in results for i in range(r.num_images)]


def regions(fn, n_regions, calls):
    fn()
    per_call = []
    for _ in range(n_regions):
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        per_call.append((time.perf_counter() - t) * 1e3 / calls)
    return {"ms": round(statistics.median(per_call), 4), "min_max": [round(min(per_call), 4), round(max(per_call), 4)]}


def upload_interval(ctx, fn, n):
    ms = (C.c_double * 6)()
    A.lib().akz_debug_match_pairs_split(ctx._h, 1, None)
    got = []
    for _ in range(n):
        fn()
        A.lib().akz_debug_match_pairs_split(ctx._h, 1, ms)
        got.append(ms[0])
    A.lib().akz_debug_match_pairs_split(ctx._h, 0, None)
    return round(statistics.median(got), 4)


def parent_rows(n_regions, calls):
    """(child) the flow on the build under --pkg, which has no bank"""
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    opt = options()
    rows = []
    for name, n_sets, pairs in WORKLOADS:
        results = extract(ctx, n_sets)
        rows.append({"workload": name, **regions(lambda: ctx.match_features_seeded_pairs(host_copies(results), pairs, opt), n_regions, calls)})
        for r in results:
            r.close()
    ctx.close()
    return rows


def as_bytes(rows):
    return [tuple(None if v is None else v if isinstance(v, int) else np.ascontiguousarray(v).tobytes() for v in row) for row in rows]


def workload(ctx, name, n_sets, pairs, n_regions, calls):
    import torch
    opt = options()
    results = extract(ctx, n_sets)
    feats = host_copies(results)
    bank = ctx.feature_bank(results)
    info = bank.info()
    row = {"workload": name, "sets": n_sets, "pairs": len(pairs), "rows": info["rows"], "rows_per_set": round(info["rows"] / n_sets, 1),
           "bank_bytes": info["rows"] * 72, "regions": n_regions, "calls_per_region": calls}

    def bank_flow():
        b = ctx.feature_bank(results)
        res = ctx.match_features_seeded_pairs(b, pairs, opt)
        b.close()
        return res

    legs = {"flow": lambda: ctx.match_features_seeded_pairs(host_copies(results), pairs, opt),
            "sets_call": lambda: ctx.match_features_seeded_pairs(feats, pairs, opt),
            "bank_flow": bank_flow,
            "bank_call": lambda: ctx.match_features_seeded_pairs(bank, pairs, opt),
            "bank_create": lambda: ctx.feature_bank(results).close(),
            "bank_create_from_sets": lambda: ctx.feature_bank(feats).close()}
    for leg, fn in legs.items():
        row[leg] = regions(fn, n_regions, calls)
    row["equal"] = as_bytes(legs["bank_call"]()) == as_bytes(legs["sets_call"]()) == as_bytes(bank_flow())
    row["upload_ms"] = upload_interval(ctx, legs["sets_call"], n_regions * calls)
    row["bank_call_upload_ms"] = upload_interval(ctx, legs["bank_call"], n_regions * calls)
    # the launch alone against a device-to-device copy of the same bytes
    ctx.set_profiling(1)
    ctx.kernel_rows(reset=True)
    gather = []
    for _ in range(n_regions * calls):
        ctx.feature_bank(results).close()
        got = [r for r in ctx.kernel_rows(reset=True) if r["kernel"] == "k_bank_gather"]
        assert len(got) == 1 and got[0]["launches"] == 1, got
        gather.append(got[0]["ms"])
    ctx.set_profiling(0)
    src = torch.randint(0, 255, (info["rows"], 64), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    d2d = []
    for _ in range(n_regions * calls + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        d2d.append(a.elapsed_time(b))
    row["gather_ms"] = round(statistics.median(gather), 4)
    row["d2d_ms"] = round(statistics.median(d2d[1:]), 4)
    row["gather_GBps_read_plus_write"] = round(2 * info["rows"] * 64 / (row["gather_ms"] * 1e-3) / 1e9, 1) if row["gather_ms"] > 0 else None
    row["bank_flow_over_flow"] = round(row["bank_flow"]["ms"] / row["flow"]["ms"], 3)
    row["bank_call_over_sets_call"] = round(row["bank_call"]["ms"] / row["sets_call"]["ms"], 3)
    bank.close()
    for r in results:
        r.close()
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--baseline", help="akaze-rust_amd directory of the parent build: its flow is the `parent_flow` leg")
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
            row["bank_flow_over_parent_flow"] = round(row["bank_flow"]["ms"] / par["ms"], 3)
            row["bank_call_over_parent_flow"] = round(row["bank_call"]["ms"] / par["ms"], 3)
            row["bank_flow_slower_than_parent_flow"] = bool(row["bank_flow"]["ms"] > par["ms"])
    doc = {"tool": "tools/feature_bank.py", "device": torch.cuda.get_device_name(0), "trials": TRIALS, "ratio": RATIO, "epsilon_px": EPS,
           "refine_iterations": FITS, "confidence": CONFIDENCE, "model_kind": "AKZ_RANSAC_FUNDAMENTAL_NORMALISED", "workloads": rows}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
