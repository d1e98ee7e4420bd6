#!/usr/bin/env python3
"""akz_match_features_seeded_pairs against the pairs calls that draw on the host, on the workloads of tools/match_pairs.py.

    timeout -k 10 900 python tools/seeded_ransac.py [--reps 5] [--baseline OTHER/akaze-rust_amd] [--rounds 2] [--out FILE]

Workloads, from synth_frame features of one scene with shifts: a lone 1080p pair and the exhaustive ordered pairs of 8 and 16
frames at 1920x1080, for every model kind, at 1 000 trials, ratio 0.86; epsilon 3.0 for the fundamental matrix (algebraic) and the
homography, 2.0 px for the normalised fundamental matrix (AKZ_RANSAC_FUNDAMENTAL_NORMALISED, a Sampson distance).  Per workload
three legs alternate rep by rep (medians of --reps after one warm-up, with min / max): `host_draws`,
akz_match_features_fundamental_pairs / akz_match_features_homography_pairs -- the calls that draw on the calling thread, reseeded
before every rep; the normalised kind has no such call and no such leg --; `seeded_c0`, the seeded call at confidence 0 (exactly
1 000 trials per pair: the same trial arithmetic, no host draws); `seeded_c99`, the seeded call at confidence 0.99.  Reported
beside the times: trials_run min / median / max over the pairs with K matches or more, the kept-list sizes of each leg, and the
akz_debug_match_pairs_split of each leg from timed runs of their own (for the seeded legs `host_draws` is the host's stopping
table and `trials` the rounds).  `claim`: seeded_c0 no slower than host_draws within the legs' own min / max spread, on the two
exhaustive workloads.
`normalised_against_fundamental`, per workload: the rounds' time per round at confidence 0 (the `trials` interval over the 8
rounds of 1 000 trials) of the normalised kind over the fundamental kind's of the same build; the whole call at confidence 0.99
of the two with trials_run and kept lists, and whether the normalised kind is no slower within the two legs' spread.
--baseline: every measurement of the fundamental and the homography kind runs in a child process of its own, --rounds times this
build and the other one in turn; `baseline` holds, per workload, model and seeded leg, the per-round medians of both, the ratio of
their medians and whether they agree within the spread of the rounds.  Prints one JSON document (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "akaze-rust_amd")
if "--pkg" in sys.argv:  # a child of --baseline: the build under PKG (its library and its binding), set before the import
    PKG = os.path.abspath(sys.argv[sys.argv.index("--pkg") + 1])
    os.environ["AKAZE_HIP_LIB"] = os.path.join(PKG, "libakaze_hip.so")
sys.path.insert(0, os.path.join(PKG, "python"))
import akaze_amd as A  # noqa: E402

TRIALS, RATIO = 1000, 0.86
SPLIT = ["uploads", "scans", "host_draws", "trials", "pick_filter", "readback"]
# model kind, matches per sample, epsilon_inliers
KIND = {"fundamental": (A.GUIDED_FUNDAMENTAL, 8, 3.0), "homography": (A.GUIDED_HOMOGRAPHY, 4, 3.0)}
if hasattr(A, "RANSAC_FUNDAMENTAL_NORMALISED"):  # (a --baseline build may be older)
    KIND["normalised"] = (A.RANSAC_FUNDAMENTAL_NORMALISED, 8, 2.0)


def features(ctx, w, h, n, idx=31):
    out = []
    for i in range(n):
        r = ctx.extract_features(A.synth_frame(w, h, idx, shift=(5 * i, 3 * i)), keep_all_planes=False)
        out.append((r.keypoints(), r.descriptors()))
    return out


def timed(fn):
    A.random_seed(42, 69)
    t = time.perf_counter()
    res = fn()
    return (time.perf_counter() - t) * 1e3, res


def workload(ctx, name, model, feats, pairs, reps):
    kind, k, eps = KIND[model]
    host = {"fundamental": ctx.match_features_fundamental_pairs, "homography": ctx.match_features_homography_pairs}.get(model)
    opt0 = A.RansacOptions(model_kind=kind, lowes_ratio=RATIO, max_trials=TRIALS, epsilon_inliers=eps, confidence=0.0)
    opt99 = opt0.copy(confidence=0.99)
    legs = {"seeded_c0": lambda: ctx.match_features_seeded_pairs(feats, pairs, opt0),
            "seeded_c99": lambda: ctx.match_features_seeded_pairs(feats, pairs, opt99)}
    if host:  # (first, as before)
        legs = {"host_draws": lambda: host(feats, pairs, RATIO, TRIALS, eps), **legs}
    res = {leg: timed(fn)[1] for leg, fn in legs.items()}  # warm-up, and the results
    t = {leg: [] for leg in legs}
    for _ in range(reps):
        for leg, fn in legs.items():
            t[leg].append(timed(fn)[0])
    split = {leg: [] for leg in legs}
    A.lib().akz_debug_match_pairs_split(ctx._h, 1, None)
    ms = (C.c_double * 6)()
    for _ in range(reps):
        for leg, fn in legs.items():
            timed(fn)
            A.lib().akz_debug_match_pairs_split(ctx._h, 1, ms)
            split[leg].append(list(ms))
    A.lib().akz_debug_match_pairs_split(ctx._h, 0, None)
    raw = [len(ctx.descriptor_match(feats[x][1], feats[y][1], 10000, RATIO)) for x, y in pairs]
    running = [p for p, r in enumerate(raw) if r >= k]
    row = {"workload": name, "model": model, "epsilon": eps, "pairs": len(pairs), "matches_per_pair_median": statistics.median(raw),
           "pairs_with_k_matches": len(running), "runs": reps}
    for leg in legs:
        row[leg + "_ms"] = round(statistics.median(t[leg]), 3)
        row[leg + "_ms_min_max"] = [round(min(t[leg]), 3), round(max(t[leg]), 3)]
        row[leg + "_kept_median"] = statistics.median(len(r[0]) for r in res[leg])
        row[leg + "_found"] = sum(r[1] is not None for r in res[leg])
        row[leg + "_split_ms"] = {key: round(statistics.median(s[i] for s in split[leg]), 3) for i, key in enumerate(SPLIT)}
    for leg in ("seeded_c0", "seeded_c99"):
        runs = [res[leg][p][3] for p in running] or [0]
        row[leg + "_trials_run_min_median_max"] = [min(runs), statistics.median(runs), max(runs)]
    if host:
        row["seeded_c0_over_host_draws"] = round(row["seeded_c0_ms"] / row["host_draws_ms"], 3)
        row["seeded_c99_over_host_draws"] = round(row["seeded_c99_ms"] / row["host_draws_ms"], 3)
        # no slower within the spread: the medians differ by no more than the larger min .. max range of the two legs
        spread = max(max(t[leg]) - min(t[leg]) for leg in ("host_draws", "seeded_c0"))
        row["claim_c0_no_slower"] = bool(row["seeded_c0_ms"] <= row["host_draws_ms"] + spread)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def normalised_against_fundamental(rows):
    """the new kind beside the fundamental kind of the same build, per workload"""
    out = []
    rounds = (TRIALS + A.RANSAC_ROUND - 1) // A.RANSAC_ROUND
    for n in (r for r in rows if r["model"] == "normalised"):
        f = next(r for r in rows if r["model"] == "fundamental" and r["workload"] == n["workload"])
        per_round = [r["seeded_c0_split_ms"]["trials"] / rounds for r in (n, f)]
        spread = max(r["seeded_c99_ms_min_max"][1] - r["seeded_c99_ms_min_max"][0] for r in (n, f))
        out.append({"workload": n["workload"], "rounds_at_confidence_0": rounds,
                    "round_ms_normalised": round(per_round[0], 4), "round_ms_fundamental": round(per_round[1], 4),
                    "round_ratio": round(per_round[0] / per_round[1], 3),
                    "c0_ms_normalised": n["seeded_c0_ms"], "c0_ms_fundamental": f["seeded_c0_ms"],
                    "c99_ms_normalised": n["seeded_c99_ms"], "c99_ms_fundamental": f["seeded_c99_ms"],
                    "c99_ratio": round(n["seeded_c99_ms"] / f["seeded_c99_ms"], 3),
                    "c99_trials_run_normalised": n["seeded_c99_trials_run_min_median_max"],
                    "c99_trials_run_fundamental": f["seeded_c99_trials_run_min_median_max"],
                    "c99_kept_median_normalised": n["seeded_c99_kept_median"], "c99_kept_median_fundamental": f["seeded_c99_kept_median"],
                    "c0_kept_median_normalised": n["seeded_c0_kept_median"], "c0_kept_median_fundamental": f["seeded_c0_kept_median"],
                    "claim_c99_no_slower": bool(n["seeded_c99_ms"] <= f["seeded_c99_ms"] + spread)})
    return out


def against_baseline(baseline, rounds, reps):
    """kinds F and H of this build and of the build under `baseline`, each measurement in a child process, in turn"""
    runs = {"this": [], "baseline": []}
    for _ in range(rounds):
        for who, pkg in (("this", PKG), ("baseline", baseline)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--kinds", "fundamental,homography", "--reps",
                                  str(reps), "--rows"], check=True, stdout=subprocess.PIPE, timeout=600).stdout
            runs[who].append(json.loads(out))
    table = []
    for i, first in enumerate(runs["this"][0]):
        for leg in ("seeded_c0", "seeded_c99", "host_draws"):
            ms = {who: [r[i][leg + "_ms"] for r in runs[who]] for who in runs}
            med = {who: statistics.median(v) for who, v in ms.items()}
            spread = max(max(v) - min(v) for v in ms.values())
            table.append({"workload": first["workload"], "model": first["model"], "leg": leg, "this_ms": ms["this"], "baseline_ms": ms["baseline"],
                          "ratio": round(med["this"] / med["baseline"], 3), "spread_ms": round(spread, 3),
                          "within_spread": bool(abs(med["this"] - med["baseline"]) <= spread),
                          "within_2_percent": bool(med["this"] <= 1.02 * med["baseline"])})
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--kinds", default=",".join(KIND), help="model kinds to measure")
    ap.add_argument("--baseline", help="akaze-rust_amd directory of a build to compare kinds F and H against")
    ap.add_argument("--rounds", type=int, default=2, help="with --baseline: child processes per build")
    ap.add_argument("--pkg", help="(child) the akaze-rust_amd directory of the build to measure")
    ap.add_argument("--rows", action="store_true", help="(child) print the workloads' rows alone")
    args = ap.parse_args()
    base = against_baseline(os.path.abspath(args.baseline), args.rounds, args.reps) if args.baseline else None  # (before this process opens the GPU)
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    f1080 = features(ctx, 1920, 1080, 16)
    jobs = [("1 pair 1080p", f1080[:2], [(0, 1)]),
            ("exhaustive 8 x 1080p", f1080[:8], [(a, b) for a in range(8) for b in range(8) if a != b]),
            ("exhaustive 16 x 1080p", f1080[:16], [(a, b) for a in range(16) for b in range(16) if a != b])]
    rows = [workload(ctx, name, model, feats, pairs, args.reps) for name, feats, pairs in jobs for model in args.kinds.split(",")]
    if args.rows:
        print(json.dumps(rows))
        ctx.close()
        return
    doc = {"tool": "tools/seeded_ransac.py", "device": torch.cuda.get_device_name(0), "trials": TRIALS, "ratio": RATIO,
           "notes": ["host_draws is THIS build's akz_match_features_fundamental_pairs / _homography_pairs: the calls that draw on the "
                     "calling thread; the normalised kind exists in the seeded family only and has no such leg",
                     "epsilon 3.0 for the fundamental matrix and the homography, as tools/match_pairs.py has it; for the fundamental "
                     "matrix that is the algebraic |p1^T F p0| at unit norm, far above the options' default 0.02, and nearly every "
                     "match passes it; the normalised kind's 2.0 is a Sampson distance in pixels"],
           "workloads": rows, "normalised_against_fundamental": normalised_against_fundamental(rows)}
    if base is not None:
        doc["baseline"] = base
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
