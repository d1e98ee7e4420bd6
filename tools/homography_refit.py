#!/usr/bin/env python3
"""What the refit stage costs: akz_match_features_homography_refined with 1 and with 8 iterations against
akz_match_features_homography of the same build, on the same inputs and seed.

    timeout -k 10 1100 python tools/homography_refit.py [--baseline OTHER/akaze-rust_amd] [--rounds 7] [--reps 5] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/homography_refit.py --trace

Workloads of tools/homography_ransac.py (synth_frame features of one scene with shifts; 1 000 trials, epsilon 3.0, ratio
0.86), as four cases: one 1080p pair (the single call), four 4K pairs with one single call each, the same four in one pairs
call, and the 240 ordered pairs of 16 1080p frames in one pairs call.  Per case the median of --reps calls after a warm-up,
and for the pairs calls the pick / filter interval of akz_debug_match_pairs_split, which holds the refit kernel.

Every measurement runs in a child process of its own; a round runs, in this order, the unrefined call, 1 iteration, 8
iterations and the unrefined call again (the baseline against itself: the spread, i.e. the noise floor).  The report holds
the medians over --rounds rounds, the ratios refined / unrefined and the spread.  Prints one JSON document (and writes it to
--out if given).  --baseline: every leg also runs on that build, right before this build's, and the report adds the ratios this
build / baseline and the baseline's unrefined call against itself.  --trace: one pass of every call."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIALS, EPS, RATIO = 1000, 3.0, 0.86
CASES = ("1 pair 1080p", "4K pairs, single calls", "4K pairs, pairs call", "exhaustive 16 x 1080p")


def child(pkg, its, reps):
    sys.path.insert(0, os.path.join(pkg, "python"))
    import akaze_amd as A
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)

    def feats(w, h, n, idx=31):
        out = []
        for i in range(n):
            r = ctx.extract_features(A.synth_frame(w, h, idx, shift=(5 * i, 3 * i)), keep_all_planes=False)
            out.append((r.keypoints(), r.descriptors()))
        return out
    f1080, f4k = feats(1920, 1080, 16), feats(3840, 2160, 3)
    p4k = [(0, 1), (1, 2), (0, 2), (2, 0)]
    p240 = [(a, b) for a in range(16) for b in range(16) if a != b]
    if its is None:
        single = lambda f, a, b: A.match_features_homography(f[a][0], f[a][1], f[b][0], f[b][1], RATIO, TRIALS, EPS, ctx=ctx)
        pairs = lambda f, p: ctx.match_features_homography_pairs(f, p, RATIO, TRIALS, EPS)
    else:
        single = lambda f, a, b: A.match_features_homography_refined(f[a][0], f[a][1], f[b][0], f[b][1], RATIO, TRIALS, EPS, its, ctx=ctx)
        pairs = lambda f, p: ctx.match_features_homography_refined_pairs(f, p, RATIO, TRIALS, EPS, its)
    jobs = [(CASES[0], lambda: single(f1080, 0, 1), False),
            (CASES[1], lambda: [single(f4k, a, b) for a, b in p4k], False),
            (CASES[2], lambda: pairs(f4k, p4k), True),
            (CASES[3], lambda: pairs(f1080, p240), True)]

    def timed(fn):
        A.random_seed(42, 69)
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fn()
        return (time.perf_counter() - t) * 1e3, res
    rows = {}
    ms = (C.c_double * 6)()
    for name, fn, is_pairs in jobs:
        for _ in range(2):  # warm-up
            timed(fn)
        t = [timed(fn)[0] for _ in range(reps)]
        row = {"ms": statistics.median(t)}
        if is_pairs:
            A.lib().akz_debug_match_pairs_split(ctx._h, 1, None)
            pick = []
            for _ in range(reps):
                timed(fn)
                A.lib().akz_debug_match_pairs_split(ctx._h, 1, ms)
                pick.append(ms[4])
            A.lib().akz_debug_match_pairs_split(ctx._h, 0, None)
            row["pick_filter_refit_ms"] = statistics.median(pick)
            res = timed(fn)[1]
            row["found"] = sum(r[1] is not None for r in res)
            row["kept"] = sum(len(r[0]) for r in res)
            if its is not None:
                row["fits"] = sum(r[2] for r in res)
        rows[name] = row
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="akaze-rust_amd directory of a build to compare against")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("PKG", "ITERATIONS"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    here = os.path.join(ROOT, "akaze-rust_amd")
    if args.child:
        print(json.dumps(child(args.child[0], None if args.child[1] == "none" else int(args.child[1]), args.reps)))
        return
    if args.trace:
        for its in (None, 1, 8):
            child(here, its, 1)
        return
    legs = []
    for key, its in (("unrefined", "none"), ("refined_1", "1"), ("refined_8", "8"), ("unrefined_again", "none")):
        if args.baseline:
            legs.append(("base_" + key, args.baseline, its))
        legs.append((key, here, its))
    runs = {k: [] for k, _, _ in legs}
    for r in range(args.rounds):
        for key, pkg, its in legs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pkg, its, "--reps", str(args.reps)], check=True,
                                 capture_output=True, text=True, timeout=300).stdout
            runs[key].append(json.loads(out.strip().splitlines()[-1]))
            print(f"round {r} {key}: {runs[key][-1]}", file=sys.stderr, flush=True)
    med = {key: {wl: {m: statistics.median(x[wl][m] for x in runs[key]) for m in runs[key][0][wl]} for wl in CASES} for key in runs}
    ratios = {}
    for wl in CASES:
        base = med["unrefined"][wl]
        row = {"refined_1_over_unrefined": round(med["refined_1"][wl]["ms"] / base["ms"], 3),
               "refined_8_over_unrefined": round(med["refined_8"][wl]["ms"] / base["ms"], 3),
               "unrefined_self_spread": round(abs(med["unrefined_again"][wl]["ms"] / base["ms"] - 1.0), 3)}
        if "pick_filter_refit_ms" in base:
            row["pick_filter_refit_ms"] = {k: round(med[k][wl]["pick_filter_refit_ms"], 4) for k in med}
        if args.baseline:
            for k in ("unrefined", "refined_1", "refined_8"):
                row[f"{k}_over_base"] = round(med[k][wl]["ms"] / med["base_" + k][wl]["ms"], 3)
            row["base_unrefined_again_over_base"] = round(med["base_unrefined_again"][wl]["ms"] / med["base_unrefined"][wl]["ms"], 3)
        ratios[wl] = row
    import torch
    doc = {"tool": "tools/homography_refit.py", "device": torch.cuda.get_device_name(0), "trials": TRIALS, "epsilon": EPS,
           "ratio": RATIO, "rounds": args.rounds, "reps_per_child": args.reps, "medians": med, "ratios": ratios, "runs": runs}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
