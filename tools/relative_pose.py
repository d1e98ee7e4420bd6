#!/usr/bin/env python3
"""akz_match_features_seeded_pose_pairs against the flow it replaces, on the workloads of tools/seeded_ransac.py.

    timeout -k 10 900 python tools/relative_pose.py [--reps 7] [--baseline OTHER/akaze-rust_amd] [--out FILE]

Time.  Workloads: synth_frame features of one scene with shifts at 1920x1080 -- a lone pair and the exhaustive ordered pairs of 8
and 16 frames (1, 56 and 240 pairs) --, the normalised fundamental matrix (model_kind 3) at 2 px with two refit iterations, 1 000
trials, ratio 0.86, at confidence 0 and 0.99, one camera (f = 1200 px, centre of the frame) per set.  Per workload and stopping mode
the legs alternate rep by rep (medians of --reps after one warm-up, with min / max):
  `pose`    the new call, with the points;
  `plain`   akz_match_features_seeded_pairs of THIS build with the same options;
  `flow`    what the new call replaces: that call followed by akz_recover_pose_host per pair on the calling thread;
  `parent`  with --baseline: akz_match_features_seeded_pairs of the build under that directory, measured in a child process of its
            own before this process opens the GPU (the stage's cost is `pose` against it).
`stage_span_ms`: the pick / filter interval of akz_debug_match_pairs_split -- two events around k_pairs_pick_filter, k_refit and,
in the new call, k_pairs_pose -- of the new call minus the plain call's, medians of timed runs of their own.
Quality.  24 two-view scenes of tests/pose_numpy.py (1 000 planted matches, 0.7 px of noise, 20 % outliers), kind 3 with the
refit: rotation error (the angle of R R_true^T) and translation-direction error (the angle between t and t_true) in degrees,
median and worst, and the share of the scene's matches that the call keeps.  Recorded, not asserted.
Prints one JSON document (and writes it to --out)."""
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

TRIALS, RATIO, EPS, FITS = 1000, 0.86, 2.0, 2
CAMERA = (1200.0, 1200.0, 960.0, 540.0)
SPLIT = ["uploads", "scans", "host_draws", "trials", "pick_filter", "readback"]


def features(ctx, n, idx=31):
    out = []
    for i in range(n):
        r = ctx.extract_features(A.synth_frame(1920, 1080, idx, shift=(5 * i, 3 * i)), keep_all_planes=False)
        out.append((r.keypoints(), r.descriptors()))
    return out


def jobs(ctx):
    f = features(ctx, 16)
    return [("1 pair 1080p", f[:2], [(0, 1)]),
            ("exhaustive 8 x 1080p", f[:8], [(a, b) for a in range(8) for b in range(8) if a != b]),
            ("exhaustive 16 x 1080p", f[:16], [(a, b) for a in range(16) for b in range(16) if a != b])]


def options(confidence):
    return A.RansacOptions(model_kind=A.RANSAC_FUNDAMENTAL_NORMALISED, lowes_ratio=RATIO, max_trials=TRIALS, epsilon_inliers=EPS,
                           confidence=confidence, refine_iterations=FITS)


def clock(fn):
    t = time.perf_counter()
    res = fn()
    return (time.perf_counter() - t) * 1e3, res


def median_legs(legs, reps):
    for fn in legs.values():
        fn()
    t = {leg: [] for leg in legs}
    for _ in range(reps):
        for leg, fn in legs.items():
            t[leg].append(clock(fn)[0])
    return {leg: {"ms": round(statistics.median(v), 3), "min_max": [round(min(v), 3), round(max(v), 3)]} for leg, v in t.items()}


def parent_rows(reps):
    """(child) the plain call of the build under --pkg on every workload and stopping mode"""
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    rows = []
    for name, feats, pairs in jobs(ctx):
        for conf in (0.0, 0.99):
            opt = options(conf)
            rows.append({"workload": name, "confidence": conf,
                         **median_legs({"parent": lambda: ctx.match_features_seeded_pairs(feats, pairs, opt)}, reps)["parent"]})
    ctx.close()
    return rows


def workload(ctx, name, feats, pairs, conf, reps):
    opt = options(conf)
    cams = [CAMERA] * len(feats)

    def flow():
        res = ctx.match_features_seeded_pairs(feats, pairs, opt)
        return [A.recover_pose_host(feats[a][0], feats[b][0], m, f, CAMERA, CAMERA, points=True) if f is not None else None
                for (a, b), (m, f, it, tr) in zip(pairs, res)]
    legs = {"pose": lambda: ctx.match_features_seeded_pose_pairs(feats, cams, pairs, opt, points=True),
            "plain": lambda: ctx.match_features_seeded_pairs(feats, pairs, opt), "flow": flow}
    row = {"workload": name, "confidence": conf, "pairs": len(pairs), "runs": reps, **median_legs(legs, reps)}
    ms = (C.c_double * 6)()
    split = {"pose": [], "plain": []}
    A.lib().akz_debug_match_pairs_split(ctx._h, 1, None)
    for _ in range(reps):
        for leg in split:
            legs[leg]()
            A.lib().akz_debug_match_pairs_split(ctx._h, 1, ms)
            split[leg].append(list(ms))
    A.lib().akz_debug_match_pairs_split(ctx._h, 0, None)
    for leg in split:
        row[leg + "_split_ms"] = {key: round(statistics.median(s[i] for s in split[leg]), 4) for i, key in enumerate(SPLIT)}
    row["stage_span_ms"] = round(row["pose_split_ms"]["pick_filter"] - row["plain_split_ms"]["pick_filter"], 4)
    got, exp = legs["pose"](), flow()
    row["poses_found"] = sum(int(g[4].found) for g in got)
    row["kept_median"] = statistics.median(len(g[0]) for g in got)
    row["equals_flow"] = all((e is None and not g[4].found and not g[4].words().any()) or
                             (e is not None and np.array_equal(g[0], e[0]) and np.array_equal(g[4].words(), e[1].words()) and
                              ((e[2] is None and g[5] is None) or np.array_equal(g[5].view(np.uint32), e[2].view(np.uint32))))
                             for g, e in zip(got, exp))
    row["pose_over_plain"] = round(row["pose"]["ms"] / row["plain"]["ms"], 3)
    row["pose_over_flow"] = round(row["pose"]["ms"] / row["flow"]["ms"], 3)
    row["pose_slower_than_flow"] = bool(row["pose"]["ms"] > row["flow"]["ms"])
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def angle_deg(c):
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def quality(ctx, scenes=24, n=1000):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pose_numpy as P
    feats, truth = [], []
    for s in range(scenes):
        sc = P.pose_scene(9000 + s, n, sigma=0.7, outliers=0.2)
        rng = np.random.default_rng(9000 + s + 7)
        perm = rng.permutation(n)
        k0, k1 = np.zeros(n, A.KEYPOINT_DTYPE), np.zeros(n, A.KEYPOINT_DTYPE)
        k0["x"], k0["y"] = sc["p0"][:, 0], sc["p0"][:, 1]
        k1["x"][perm], k1["y"][perm] = sc["q1"][:, 0], sc["q1"][:, 1]
        d0 = rng.integers(0, 256, (n, 61), dtype=np.uint8)
        d1 = np.zeros_like(d0)
        d1[perm] = d0
        feats += [(k0, d0), (k1, d1)]
        truth.append(sc)
    pairs = [(2 * s, 2 * s + 1) for s in range(scenes)]
    res = ctx.match_features_seeded_pose_pairs(feats, [CAMERA] * len(feats), pairs, options(0.99))
    rot, tra, share = [], [], []
    for (m, f, it, tr, pose), sc in zip(res, truth):
        if not pose.found:
            continue
        rot.append(angle_deg((np.trace(pose.R.astype(np.float64) @ sc["r"].T) - 1.0) / 2.0))
        tra.append(angle_deg(np.dot(pose.T.astype(np.float64), sc["t"] / np.linalg.norm(sc["t"]))))
        share.append(len(m) / n)
    return {"scenes": scenes, "matches": n, "noise_px": 0.7, "outliers": 0.2, "poses_found": len(rot),
            "rotation_error_deg_median_worst": [round(statistics.median(rot), 4), round(max(rot), 4)],
            "translation_direction_error_deg_median_worst": [round(statistics.median(tra), 4), round(max(tra), 4)],
            "kept_share_median_min": [round(statistics.median(share), 4), round(min(share), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--baseline", help="akaze-rust_amd directory of the parent build: its akz_match_features_seeded_pairs is the `parent` leg")
    ap.add_argument("--pkg", help="(child) the akaze-rust_amd directory of the build to measure")
    ap.add_argument("--rows", action="store_true", help="(child) print the parent leg's rows alone")
    args = ap.parse_args()
    if args.rows:
        print(json.dumps(parent_rows(args.reps)))
        return
    parent = None
    if args.baseline:  # (before this process opens the GPU)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", os.path.abspath(args.baseline), "--reps", str(args.reps), "--rows"],
                             check=True, stdout=subprocess.PIPE, timeout=600).stdout
        parent = json.loads(out)
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    rows = [workload(ctx, name, feats, pairs, conf, args.reps) for name, feats, pairs in jobs(ctx) for conf in (0.0, 0.99)]
    if parent:
        for row, par in zip(rows, parent):
            assert (row["workload"], row["confidence"]) == (par["workload"], par["confidence"])
            row["parent"] = {"ms": par["ms"], "min_max": par["min_max"]}
            row["stage_cost_ms"] = round(row["pose"]["ms"] - par["ms"], 3)
            row["pose_over_parent"] = round(row["pose"]["ms"] / par["ms"], 3)
    doc = {"tool": "tools/relative_pose.py", "device": torch.cuda.get_device_name(0), "trials": TRIALS, "ratio": RATIO, "epsilon_px": EPS,
           "refine_iterations": FITS, "model_kind": "AKZ_RANSAC_FUNDAMENTAL_NORMALISED",
           "notes": ["the frames of the time workloads are shifts of one scene: a pure image translation, which an exact F would "
                     "call a pure rotation; the noisy F still decomposes and the stage does its full work (counts, compaction, "
                     "points), but the poses themselves mean nothing there -- quality is measured on the two-view scenes",
                     "stage_span_ms is a difference of two event intervals that both hold the pick / filter and the refit"],
           "workloads": rows, "quality": quality(ctx)}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
