#!/usr/bin/env python3
"""akz_match_features_seeded_pairs against the pairs calls that draw on the host, on the workloads of tools/match_pairs.py.

    timeout -k 10 900 python tools/seeded_ransac.py [--reps 5] [--out profiles/r14_seeded_ransac.json]

Workloads, from synth_frame features of one scene with shifts: a lone 1080p pair and the exhaustive ordered pairs of 8 and 16
frames at 1920x1080, for both models, at 1 000 trials, epsilon 3.0, ratio 0.86.  Per workload three legs alternate rep by rep
(medians of --reps after one warm-up, with min / max): `host_draws`, akz_match_features_fundamental_pairs /
akz_match_features_homography_pairs -- the calls this addition leaves as they are, reseeded before every rep --; `seeded_c0`,
the seeded call at confidence 0 (exactly 1 000 trials per pair: the same trial arithmetic, no host draws); `seeded_c99`, the
seeded call at confidence 0.99.  Reported beside the times: trials_run min / median / max over the pairs with K matches or
more, the kept-list sizes of each leg, and the akz_debug_match_pairs_split of each leg from timed runs of their own (for the
seeded legs `host_draws` is the host's stopping table and `trials` the rounds).  `claim`: seeded_c0 no slower than host_draws
within the legs' own min / max spread, on the two exhaustive workloads.  Prints one JSON document (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akaze-rust_amd", "python"))
import akaze_amd as A  # noqa: E402

TRIALS, EPS, RATIO = 1000, 3.0, 0.86
SPLIT = ["uploads", "scans", "host_draws", "trials", "pick_filter", "readback"]
KIND = {"fundamental": (A.GUIDED_FUNDAMENTAL, 8), "homography": (A.GUIDED_HOMOGRAPHY, 4)}


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
    kind, k = KIND[model]
    host = ctx.match_features_fundamental_pairs if model == "fundamental" else ctx.match_features_homography_pairs
    opt0 = A.RansacOptions(model_kind=kind, lowes_ratio=RATIO, max_trials=TRIALS, epsilon_inliers=EPS, confidence=0.0)
    opt99 = opt0.copy(confidence=0.99)
    legs = {"host_draws": lambda: host(feats, pairs, RATIO, TRIALS, EPS),
            "seeded_c0": lambda: ctx.match_features_seeded_pairs(feats, pairs, opt0),
            "seeded_c99": lambda: ctx.match_features_seeded_pairs(feats, pairs, opt99)}
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
    row = {"workload": name, "model": model, "pairs": len(pairs), "matches_per_pair_median": statistics.median(raw),
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
    row["seeded_c0_over_host_draws"] = round(row["seeded_c0_ms"] / row["host_draws_ms"], 3)
    row["seeded_c99_over_host_draws"] = round(row["seeded_c99_ms"] / row["host_draws_ms"], 3)
    # no slower within the spread: the medians differ by no more than the larger min .. max range of the two legs
    spread = max(max(t[leg]) - min(t[leg]) for leg in ("host_draws", "seeded_c0"))
    row["claim_c0_no_slower"] = bool(row["seeded_c0_ms"] <= row["host_draws_ms"] + spread)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    args = ap.parse_args()
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    f1080 = features(ctx, 1920, 1080, 16)
    jobs = [("1 pair 1080p", f1080[:2], [(0, 1)]),
            ("exhaustive 8 x 1080p", f1080[:8], [(a, b) for a in range(8) for b in range(8) if a != b]),
            ("exhaustive 16 x 1080p", f1080[:16], [(a, b) for a in range(16) for b in range(16) if a != b])]
    rows = [workload(ctx, name, model, feats, pairs, args.reps) for name, feats, pairs in jobs for model in KIND]
    doc = {"tool": "tools/seeded_ransac.py", "device": torch.cuda.get_device_name(0), "trials": TRIALS, "epsilon": EPS, "ratio": RATIO,
           "notes": ["host_draws is THIS build's akz_match_features_fundamental_pairs / _homography_pairs: the existing calls, whose "
                     "orchestration is unchanged apart from the scan loop moved into a function",
                     "epsilon 3.0 for both models, as tools/match_pairs.py has it; for the fundamental matrix that is the algebraic "
                     "|p1^T F p0| at unit norm, far above the options' default 0.02"],
           "workloads": rows}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
