#!/usr/bin/env python3
"""What the refit of the RANSAC fundamental matrix gives and costs: accuracy against the unrefined winner of the same draws,
and the time of akz_match_features_fundamental_refined_pairs against akz_match_features_pairs (of this build and, with
--baseline, of another one) and against what a user could do before: the unrefined call, then akz_refine_fundamental_matrix on
the host for every pair.

    timeout -k 10 1100 python tools/fundamental_refit.py [--baseline OTHER/akaze-rust_amd] [--rounds 5] [--reps 5] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/fundamental_refit.py --trace

Workload: 64 pairs of planted-descriptor sets, each a two-view scene of 2 000 matches (the generator of
tests/test_fundamental_refit_host.py: 0.7 px noise, 20 % outliers), 1 000 trials, epsilon 0.02 (1 .. 5 px), ratio 0.86, 8 refit
iterations, all in one pairs call.  Per leg the median of --reps calls after a warm-up and the pick / filter interval of
akz_debug_match_pairs_split, which holds the refit kernel; refit_kernel_ms is that interval with the refit minus without.

Every measurement runs in a child process of its own; a round runs, in this order, match_features_pairs (of the baseline
first, if given), the unrefined call with the model, the refined call, the unrefined call followed by the host refit, and
match_features_pairs again (the spread).  The report holds the medians over --rounds rounds and their ratios, the accuracy of
the 64 pairs (mean symmetric epipolar distance to the noise-free correspondences, winner and refined) and the quality
figures of the test's committed scenes, computed on the host.  Prints one JSON document (and writes it to --out if given).
--trace: one pass of every call of this build.  --host-only: the quality figures alone (no GPU call, no timing)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIALS, EPS, RATIO, ITS, PAIRS, MATCHES = 1000, 0.02, 0.86, 8, 64, 2000
LEGS = ("pairs", "fundamental", "refined", "unrefined_then_host", "pairs_again")


def _scenes():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_fundamental_refit_host as T
    return T


def child(pkg, leg, reps):
    sys.path.insert(0, os.path.join(pkg, "python"))
    import akaze_amd as A
    import numpy as np
    import torch
    T = _scenes()
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    feats, scenes = [], []
    for s in range(PAIRS):
        sc = T.two_view_scene(9000 + s, MATCHES)
        rng = np.random.default_rng(19000 + s)
        perm = rng.permutation(MATCHES)
        k0, k1 = np.zeros(MATCHES, A.KEYPOINT_DTYPE), np.zeros(MATCHES, A.KEYPOINT_DTYPE)
        k0["x"], k0["y"] = sc[0][:, 0], sc[0][:, 1]
        k1["x"][perm], k1["y"][perm] = sc[2][:, 0], sc[2][:, 1]
        d0 = rng.integers(0, 256, (MATCHES, 61), dtype=np.uint8)
        d1 = np.zeros_like(d0)
        d1[perm] = d0
        feats += [(k0, d0), (k1, d1)]
        scenes.append(sc)
    pairs = [(2 * s, 2 * s + 1) for s in range(PAIRS)]

    def then_host():
        res = ctx.match_features_fundamental_pairs(feats, pairs, RATIO, TRIALS, EPS)
        out = []
        for (a, b), (kept, f) in zip(pairs, res):
            if f is None:
                out.append((kept, f, 0))
                continue
            raw = ctx.descriptor_match(feats[a][1], feats[b][1], 10000, RATIO)   # (the pairs call does not hand the raw list back)
            out.append(A.refine_fundamental_matrix(feats[a][0], feats[b][0], raw, f, EPS, ITS))
        return out
    fn = {"pairs": lambda: ctx.match_features_pairs(feats, pairs, RATIO, TRIALS, EPS),
          "pairs_again": lambda: ctx.match_features_pairs(feats, pairs, RATIO, TRIALS, EPS),
          "fundamental": lambda: ctx.match_features_fundamental_pairs(feats, pairs, RATIO, TRIALS, EPS),
          "refined": lambda: ctx.match_features_fundamental_refined_pairs(feats, pairs, RATIO, TRIALS, EPS, ITS),
          "unrefined_then_host": then_host}[leg]

    def timed():
        A.random_seed(42, 69)
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fn()
        return (time.perf_counter() - t) * 1e3, res
    for _ in range(2):  # warm-up
        timed()
    row = {"ms": statistics.median(timed()[0] for _ in range(reps))}
    ms = (C.c_double * 6)()
    A.lib().akz_debug_match_pairs_split(ctx._h, 1, None)
    pick = []
    for _ in range(reps):
        timed()
        A.lib().akz_debug_match_pairs_split(ctx._h, 1, ms)
        pick.append(ms[4])
    A.lib().akz_debug_match_pairs_split(ctx._h, 0, None)
    row["pick_filter_refit_ms"] = statistics.median(pick)
    res = timed()[1]
    if leg.startswith("pairs"):
        row["kept"] = sum(len(r) for r in res)
    else:
        row["kept"] = sum(len(r[0]) for r in res)
        row["found"] = sum(r[1] is not None for r in res)
        row["error_px"] = [None if r[1] is None else T.epipolar_error(r[1], sc[0], sc[1]) for r, sc in zip(res, scenes)]
        if len(res[0]) == 3:
            row["fits"] = sum(r[2] for r in res)
    ctx.close()
    return row


def host_quality(pkg):
    """the committed quality scenes of tests/test_fundamental_refit_host.py, on the host alone"""
    sys.path.insert(0, os.path.join(pkg, "python"))
    import akaze_amd as A
    import numpy as np
    T = _scenes()
    rows = []
    for seed, n in T.QUALITY_SCENES:
        k0, k1, m, sc = T.scene_case(A, seed, n)
        eps = T.scene_epsilon(sc[4], sc[0])
        A.random_seed(42, 69)
        kept, f = A.remove_outliers_fundamental(k0, k1, m, 500, T.EPS_MODEL, eps)
        kept2, f2, its = A.refine_fundamental_matrix(k0, k1, m, f, eps, 8)
        before, after = T.epipolar_error(f, sc[0], sc[1]), T.epipolar_error(f2, sc[0], sc[1])
        rows.append({"seed": seed, "n": n, "winner_px": before, "refined_px": after, "ratio": after / before, "winner_inliers": len(kept),
                     "refined_inliers": len(kept2), "true_inliers": int((~sc[3]).sum()), "fits": its})
    return {"scenes": rows, "median_ratio": float(np.median([r["ratio"] for r in rows]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="akaze-rust_amd directory of a build to compare against (its match_features_pairs)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("PKG", "LEG"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    here = os.path.join(ROOT, "akaze-rust_amd")
    if args.child:
        print(json.dumps(child(args.child[0], args.child[1], args.reps)))
        return
    if args.trace:
        for leg in LEGS[:4]:
            child(here, leg, 1)
        return
    if args.host_only:
        doc = {"tool": "tools/fundamental_refit.py --host-only", "timing": "not measured", "quality_host": host_quality(here)}
        txt = json.dumps(doc, indent=1)
        print(txt)
        if args.out:
            with open(args.out, "w") as f:
                f.write(txt + "\n")
        return
    legs = []
    for leg in LEGS:
        if args.baseline and leg.startswith("pairs"):
            legs.append(("base_" + leg, args.baseline, leg))
        legs.append((leg, here, leg))
    runs = {k: [] for k, _, _ in legs}
    for r in range(args.rounds):
        for key, pkg, leg in legs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pkg, leg, "--reps", str(args.reps)], check=True,
                                 capture_output=True, text=True, timeout=300).stdout
            runs[key].append(json.loads(out.strip().splitlines()[-1]))
            print(f"round {r} {key}: ms {runs[key][-1]['ms']:.3f} pick {runs[key][-1]['pick_filter_refit_ms']:.4f}", file=sys.stderr, flush=True)
    med = {key: {m: statistics.median(x[m] for x in runs[key]) for m in ("ms", "pick_filter_refit_ms")} for key in runs}
    ratios = {"refined_over_pairs": round(med["refined"]["ms"] / med["pairs"]["ms"], 3),
              "refined_over_unrefined_with_model": round(med["refined"]["ms"] / med["fundamental"]["ms"], 3),
              "refined_over_unrefined_then_host": round(med["refined"]["ms"] / med["unrefined_then_host"]["ms"], 3),
              "unrefined_with_model_over_pairs": round(med["fundamental"]["ms"] / med["pairs"]["ms"], 3),
              "pairs_self_spread": round(abs(med["pairs_again"]["ms"] / med["pairs"]["ms"] - 1.0), 3),
              "refit_kernel_ms": round(med["refined"]["pick_filter_refit_ms"] - med["fundamental"]["pick_filter_refit_ms"], 4)}
    if args.baseline:
        ratios["refined_over_base_pairs"] = round(med["refined"]["ms"] / med["base_pairs"]["ms"], 3)
        ratios["pairs_over_base_pairs"] = round(med["pairs"]["ms"] / med["base_pairs"]["ms"], 3)
        ratios["base_pairs_self_spread"] = round(abs(med["base_pairs_again"]["ms"] / med["base_pairs"]["ms"] - 1.0), 3)
    # accuracy of the 64 pairs: the winner (the unrefined call) against the refined F of the same draws
    win, ref = runs["fundamental"][0]["error_px"], runs["refined"][0]["error_px"]
    both = [(w, r) for w, r in zip(win, ref) if w is not None and r is not None]
    usable = [(w, r) for w, r in both if w < 2.0]
    accuracy = {"pairs_with_a_model": len(both), "winner_within_2_px": len(usable),
                "median_ratio_where_winner_within_2_px": statistics.median(r / w for w, r in usable) if usable else None,
                "median_ratio_all": statistics.median(r / w for w, r in both) if both else None,
                "refined_worse": sum(r > w for w, r in both), "winner_px": win, "refined_px": ref,
                "kept": {k: runs[k][0]["kept"] for k in ("pairs", "fundamental", "refined", "unrefined_then_host")},
                "fits": runs["refined"][0].get("fits"),
                "device_equals_host_errors": runs["refined"][0]["error_px"] == runs["unrefined_then_host"][0]["error_px"]}
    import torch
    doc = {"tool": "tools/fundamental_refit.py", "device": torch.cuda.get_device_name(0), "pairs": PAIRS, "matches_per_pair": MATCHES,
           "trials": TRIALS, "epsilon": EPS, "ratio": RATIO, "refine_iterations": ITS, "rounds": args.rounds, "reps_per_child": args.reps,
           "medians": med, "ratios": ratios, "accuracy": accuracy, "quality_host": host_quality(here),
           "runs": {k: [{m: v for m, v in x.items() if m != "error_px"} for x in runs[k]] for k in runs}}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
