#!/usr/bin/env python3
"""akz_resection_seeded_problems against the host statement looped on one thread, and a resection round against a round of the
normalised fundamental matrix.

    timeout -k 10 900 python tools/resection.py [--out profiles/r32_resection.json]

Time (the README's method: medians of five regions of 20 synchronous calls).  Workloads: 1, 56 and 240 problems of 1 000
correspondences -- the scenes of tests/resection_numpy.py with 0.7 px of noise and 20 % outliers, judged at 3 px -- 1 000 trials,
two refit iterations, at confidence 0 and 0.99.  Per workload:
  `gpu`        the call through the ABI on arguments packed once;
  `host_loop`  akz_resection_seeded_host over the problems on the calling thread, ONE pass (240 problems of 1 000 trials take
               seconds);
  `split_ms`   akz_debug_resection_split of timed calls of their own: upload, rounds, filter + refit, read-back, and from it the
               cost of a round (rounds / the rounds the call launched) and the read-back's share of the four;
  `f3_round_ms` the same per-round cost of akz_match_features_seeded_pairs with AKZ_RANSAC_FUNDAMENTAL_NORMALISED on as many pairs
               of 1 000 planted matches (the `trials` interval of akz_debug_match_pairs_split / rounds): kind 3's kernels are the
               parent commit's, byte for byte in the compiler's resource report.
Quality.  24 such scenes at 0.7 px and at 1.5 px of noise, eps 2, 3, 4 and 6 px, 1 000 trials, confidence 0.99, two refit
iterations: rotation error (the angle of R R_true^T, degrees), translation error (|t - t_true| / |t_true|), the share of the true
correspondences kept and the outliers kept -- median and worst -- and the winners' kept share before the refit.  Recorded, not
asserted.  Prints one JSON document (and writes it to --out)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import akaze_amd as A  # noqa: E402
import resection_numpy as rn  # noqa: E402

TRIALS, FITS, EPS, NOISE, N = 1000, 2, 3.0, 0.7, 1000
REGIONS, CALLS = 5, 20


def scenes(count, noise=NOISE, base=7000):
    return [rn.make_scene(base + s, N - N // 5, N // 5, noise=noise) for s in range(count)]


def options(confidence, eps=EPS, fits=FITS, trials=TRIALS, kind=None):
    return A.RansacOptions(model_kind=A.RANSAC_RESECTION if kind is None else kind, max_trials=trials, epsilon_inliers=eps,
                           confidence=confidence, refine_iterations=fits)


def regions(fn):
    """-> median, min, max over REGIONS of the mean ms per call of CALLS synchronous calls"""
    fn()
    per = []
    for _ in range(REGIONS):
        t = time.perf_counter()
        for _ in range(CALLS):
            fn()
        per.append((time.perf_counter() - t) * 1e3 / CALLS)
    return {"ms": round(statistics.median(per), 4), "min_max": [round(min(per), 4), round(max(per), 4)]}


def planted_pairs(count):
    """`count` pairs of 1 000 planted matches with 20 % outliers for the kind-3 call (random descriptors, permuted)"""
    import pose_numpy as P
    feats = []
    for s in range(count):
        sc = P.pose_scene(9000 + s, N, sigma=NOISE, outliers=0.2)
        rng = np.random.default_rng(9000 + s + 7)
        perm = rng.permutation(N)
        k0, k1 = np.zeros(N, A.KEYPOINT_DTYPE), np.zeros(N, A.KEYPOINT_DTYPE)
        k0["x"], k0["y"] = sc["p0"][:, 0], sc["p0"][:, 1]
        k1["x"][perm], k1["y"][perm] = sc["q1"][:, 0], sc["q1"][:, 1]
        d0 = rng.integers(0, 256, (N, 61), dtype=np.uint8)
        d1 = np.zeros_like(d0)
        d1[perm] = d0
        feats += [(k0, d0), (k1, d1)]
    return feats, [(2 * s, 2 * s + 1) for s in range(count)]


def workload(ctx, count, conf):
    L = A.lib()
    problems = [(sc["points"], sc["pixels"], sc["camera"]) for sc in scenes(count)]
    a = A._ResectionArgs(problems)
    opt = options(conf)

    def gpu():
        A._check(L.akz_resection_seeded_problems(ctx._h, a.problems, count, C.byref(opt), *a.tail()))
    row = {"problems": count, "confidence": conf, "gpu": regions(gpu)}
    got = a.results()
    t = time.perf_counter()
    exp = [A.resection_seeded_host(*q, opt, stream=p) for p, q in enumerate(problems)]
    row["host_loop"] = {"ms": round((time.perf_counter() - t) * 1e3, 2), "passes": 1}
    row["equals_host"] = all(np.array_equal(g[0], e[0]) and np.array_equal(g[1].words(), e[1].words()) and g[2:] == e[2:] for g, e in zip(got, exp))
    row["trials_run_median"] = statistics.median(g[3] for g in got)
    row["kept_median"] = statistics.median(len(g[0]) for g in got)
    row["host_over_gpu"] = round(row["host_loop"]["ms"] / row["gpu"]["ms"], 2)
    row["gpu_slower_than_host_loop"] = bool(row["gpu"]["ms"] > row["host_loop"]["ms"])
    ms = (C.c_double * 4)()
    L.akz_debug_resection_split(ctx._h, 1, None)
    split = []
    for _ in range(CALLS):
        gpu()
        L.akz_debug_resection_split(ctx._h, 1, ms)
        split.append(list(ms))
    L.akz_debug_resection_split(ctx._h, 0, None)
    med = [statistics.median(s[i] for s in split) for i in range(4)]
    rounds = -(-int(max(g[3] for g in got)) // A.RANSAC_ROUND)
    row["split_ms"] = dict(zip(("upload", "rounds", "filter_refit", "readback"), (round(v, 4) for v in med)))
    row["rounds_launched"] = rounds
    row["round_ms"] = round(med[1] / rounds, 4)
    row["readback_share"] = round(med[3] / sum(med), 4)
    # kind 3 on as many pairs of as many matches
    feats, pairs = planted_pairs(count)
    opt3 = A.RansacOptions(model_kind=A.RANSAC_FUNDAMENTAL_NORMALISED, lowes_ratio=0.86, max_trials=TRIALS, epsilon_inliers=2.0, confidence=conf,
                           refine_iterations=FITS)
    ms6 = (C.c_double * 6)()
    L.akz_debug_match_pairs_split(ctx._h, 1, None)
    tr, runs = [], 0
    for _ in range(CALLS):
        res = ctx.match_features_seeded_pairs(feats, pairs, opt3)
        L.akz_debug_match_pairs_split(ctx._h, 1, ms6)
        tr.append(ms6[3])
        runs = max(r[3] for r in res)
    L.akz_debug_match_pairs_split(ctx._h, 0, None)
    row["f3_round_ms"] = round(statistics.median(tr) / -(-int(runs) // A.RANSAC_ROUND), 4)
    row["round_over_f3_round"] = round(row["round_ms"] / row["f3_round_ms"], 2)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def quality(ctx, noise, eps):
    sc = scenes(24, noise, base=8000)
    problems = [(s["points"], s["pixels"], s["camera"]) for s in sc]
    res = ctx.resection_seeded(problems, options(0.99, eps))
    plain = ctx.resection_seeded(problems, options(0.99, eps, fits=0))
    rot, tra, share, outl, win = [], [], [], [], []
    for (kept, pose, its, run), (k0, _, _, _), s in zip(res, plain, sc):
        true = s["true"]
        win.append(float(true[k0].sum()) / true.sum())
        if not pose.found:
            continue
        ea, et = rn.pose_error(pose.R, pose.T, s["R"], s["t"])
        rot.append(np.degrees(ea))
        tra.append(et)
        share.append(float(true[kept].sum()) / true.sum())
        outl.append(int((~true[kept]).sum()))
    mw = lambda v, worst=max: [round(float(statistics.median(v)), 5), round(float(worst(v)), 5)]  # noqa: E731
    return {"noise_px": noise, "eps_px": eps, "scenes": 24, "found": len(rot), "rotation_error_deg_median_worst": mw(rot),
            "translation_error_median_worst": mw(tra), "true_kept_share_median_min": mw(share, min), "outliers_kept_median_max": mw(outl),
            "winner_true_share_median_min": mw(win, min)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    args = ap.parse_args()
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    rows = [workload(ctx, count, conf) for count in (1, 56, 240) for conf in (0.0, 0.99)]
    qual = [quality(ctx, noise, eps) for noise in (0.7, 1.5) for eps in (2.0, 3.0, 4.0, 6.0)]
    doc = {"tool": "tools/resection.py", "device": torch.cuda.get_device_name(0), "correspondences": N, "trials": TRIALS, "epsilon_px": EPS,
           "noise_px": NOISE, "refine_iterations": FITS, "method": f"medians of {REGIONS} regions of {CALLS} synchronous calls",
           "workloads": rows, "quality": qual}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
