#!/usr/bin/env python3
"""The homography RANSAC calls against the fundamental-matrix calls, and this build's two paths against another build's.

    timeout -k 10 900 python tools/homography_ransac.py --baseline OTHER/akaze-rust_amd [--rounds 5] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/homography_ransac.py --trace

Workloads of tools/match_pairs.py (synth_frame features of one scene with shifts, so a homography -- a translation --
explains every true match): one 1080p pair, four 4K pairs, the 240 ordered pairs of 16 1080p frames; 1 000 trials, epsilon
3.0, ratio 0.86.  Per workload: the single-pair calls in a loop (akz_match_features / akz_match_features_homography) and the
pairs call (akz_match_features_pairs / akz_match_features_homography_pairs), medians of --reps after a warm-up, plus the
pairs call's host draw time (akz_debug_match_pairs_split).

Every measurement runs in a child process of one build and one model; a round runs, in this order, the baseline's F, this
build's F, the baseline's H, this build's H and the baseline's F and H again (the baseline against itself: the spread).  The
report holds the medians over --rounds rounds, the ratios H / F (this build), F / F and H / H (this build over the baseline),
and the baseline's spread per model.  Prints one JSON document (and writes it to --out if given).  --trace: one pass of every
call of this build, both models."""
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


def child(pkg, model, reps):
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
    jobs = [("1 pair 1080p", f1080[:2], [(0, 1)]),
            ("4K pairs", f4k, [(0, 1), (1, 2), (0, 2), (2, 0)]),
            ("exhaustive 16 x 1080p", f1080, [(a, b) for a in range(16) for b in range(16) if a != b])]
    if model == "H":
        single = lambda f, a, b: A.match_features_homography(f[a][0], f[a][1], f[b][0], f[b][1], RATIO, TRIALS, EPS, ctx=ctx)
        pairs = lambda f, p: ctx.match_features_homography_pairs(f, p, RATIO, TRIALS, EPS)
    else:
        single = lambda f, a, b: A.match_features(f[a][0], f[a][1], f[b][0], f[b][1], RATIO, TRIALS, EPS, ctx=ctx)
        pairs = lambda f, p: ctx.match_features_pairs(f, p, RATIO, TRIALS, EPS)

    def timed(fn):
        A.random_seed(42, 69)
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3
    rows = {}
    ms = (C.c_double * 6)()
    for name, f, p in jobs:
        t_loop, t_pairs, draws = [], [], []
        run_loop = (lambda: [single(f, a, b) for a, b in p]) if len(p) <= 4 else None
        for _ in range(2):  # warm-up
            if run_loop:
                timed(run_loop)
            timed(lambda: pairs(f, p))
        for _ in range(reps):
            if run_loop:
                t_loop.append(timed(run_loop))
            t_pairs.append(timed(lambda: pairs(f, p)))
        A.lib().akz_debug_match_pairs_split(ctx._h, 1, None)
        for _ in range(reps):
            timed(lambda: pairs(f, p))
            A.lib().akz_debug_match_pairs_split(ctx._h, 1, ms)
            draws.append(ms[2])
        A.lib().akz_debug_match_pairs_split(ctx._h, 0, None)
        rows[name] = {"pairs": len(p), "loop_ms": statistics.median(t_loop) if t_loop else None,
                      "pairs_ms": statistics.median(t_pairs), "host_draw_ms": statistics.median(draws)}
    if model == "H":  # the trials' models: how many of them there were
        A.random_seed(42, 69)
        res = ctx.match_features_homography_pairs(f1080, jobs[2][2], RATIO, TRIALS, EPS)
        rows["exhaustive 16 x 1080p"]["found"] = sum(h is not None for _, h in res)
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="akaze-rust_amd directory of the build to compare against")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("PKG", "MODEL"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    here = os.path.join(ROOT, "akaze-rust_amd")
    if args.child:
        print(json.dumps(child(args.child[0], args.child[1], args.reps)))
        return
    if args.trace:
        child(here, "F", 1)
        child(here, "H", 1)
        return
    legs = [("base_F", args.baseline, "F"), ("F", here, "F"), ("base_H", args.baseline, "H"), ("H", here, "H"),
            ("base_F_again", args.baseline, "F"), ("base_H_again", args.baseline, "H")]
    runs = {k: [] for k, _, _ in legs}
    for r in range(args.rounds):
        for key, pkg, model in legs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pkg, model, "--reps", str(args.reps)],
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            runs[key].append(json.loads(out.strip().splitlines()[-1]))
            print(f"round {r} {key}: {runs[key][-1]}", file=sys.stderr, flush=True)
    med = {}
    for key in runs:
        med[key] = {}
        for wl in runs[key][0]:
            med[key][wl] = {m: (statistics.median(x[wl][m] for x in runs[key]) if runs[key][0][wl][m] is not None else None)
                            for m in runs[key][0][wl] if m != "pairs"}
    ratios = {}
    for wl in med["H"]:
        row = {}
        for m in ("loop_ms", "pairs_ms"):
            if med["H"][wl][m] is None:
                continue
            row[f"H_over_F_{m}"] = round(med["H"][wl][m] / med["F"][wl][m], 3)
            for k in "FH":
                row[f"{k}_over_base_{m}"] = round(med[k][wl][m] / med[f"base_{k}"][wl][m], 3)
                row[f"base_{k}_again_over_base_{m}"] = round(med[f"base_{k}_again"][wl][m] / med[f"base_{k}"][wl][m], 3)
        ratios[wl] = row
    import torch
    doc = {"tool": "tools/homography_ransac.py", "device": torch.cuda.get_device_name(0), "trials": TRIALS, "epsilon": EPS,
           "ratio": RATIO, "rounds": args.rounds, "reps_per_child": args.reps, "medians_ms": med, "ratios": ratios, "runs": runs}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
