#!/usr/bin/env python3
"""Guided matching against the blind scan, and the composite call against its two stages called one after the other.

    timeout -k 10 1100 python tools/guided_match.py [--baseline OTHER/akaze-rust_amd] [--reps 7] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/guided_match.py --trace

Shapes (synth_frame features of one scene with whole-pixel shifts, so a translation H explains every true match): the
4K pair's own sets (about 11 K x 11 K rows), a 1080p pair, and the 120 unordered pairs of 16 4K frames extracted with
5 sublevels x 5 octaves.  Per shape, medians of --reps calls after two warm-up calls, in milliseconds of wall time around
a synchronous call:
  * guided_H / guided_F   akz_descriptor_match_guided_pairs with the shift's H / F = [t]x, radius 3 (host arrays in, lists out);
  * blind                 akz_descriptor_match on the same sets, pair by pair (host arrays in, lists out: the same uploads
                          and read-backs as the guided call, so the two compare scan against scan);
  * blind_device          akz_descriptor_match_device on device-resident rows (the scan and its compaction alone);
  * composite             akz_match_features_homography_guided_pairs (1 000 trials, epsilon 3, ratio 0.86, guided 3 / 0.86);
  * two_calls             akz_match_features_homography_pairs, then akz_descriptor_match_guided_pairs over the found pairs
                          (what the composite saves: the second upload of every set).
--baseline: the blind figures of another build (the parent commit's) in a child process of its own, for the yardstick the
guided scan is held against.  Each build's child process has 500 s.  Prints one JSON document and writes it to --out
(default profiles/r09_guided.json).  Ratios: guided / blind compares calls that take host arrays and return lists (the same
uploads and read-backs on both sides); guided / blind_device holds the whole guided call against the device-resident scan
alone.  --trace: one pass of every call."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIALS, EPS, RATIO, RADIUS = 1000, 3.0, 0.86, 3.0


def shapes(A, ctx):
    def feats(w, h, n, **cfg):
        out = []
        for i in range(n):
            r = ctx.extract_features(A.synth_frame(w, h, 31, shift=(5 * i, 3 * i)), A.Config(**cfg) if cfg else None,
                                     keep_all_planes=False)
            out.append((r.keypoints(), r.descriptors()))
        return out
    f4k, f1080 = feats(3840, 2160, 2), feats(1920, 1080, 2)
    f55 = feats(3840, 2160, 16, num_sublevels=5, max_octave_evolution=5)
    return [("4K pair", f4k, [(0, 1)]), ("1080p pair", f1080, [(0, 1)]),
            ("16 x 4K 5x5, 120 pairs", f55, [(a, b) for a in range(16) for b in range(a + 1, 16)])]


def child(pkg, reps, blind_only, trace):
    sys.path.insert(0, os.path.join(pkg, "python"))
    import akaze_amd as A
    import numpy as np
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)

    def median_ms(fn):
        ts = []
        for k in range((0 if trace else 2) + (1 if trace else reps)):
            A.random_seed(42, 69)
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if trace or k >= 2:
                ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts)
    rows = {}
    for name, f, pairs in shapes(A, ctx):
        # the sign of the shift between consecutive frames, from the blind matches of the first pair
        a, b = pairs[0]
        m = ctx.descriptor_match(f[a][1], f[b][1], 10000, RATIO)
        sx = float(np.rint(np.median(f[b][0]["x"][m["index_1"]] - f[a][0]["x"][m["index_0"]]))) / (b - a)
        sy = float(np.rint(np.median(f[b][0]["y"][m["index_1"]] - f[a][0]["y"][m["index_0"]]))) / (b - a)
        hs = np.stack([np.array([[1, 0, sx * (q - p)], [0, 1, sy * (q - p)], [0, 0, 1]], np.float32) for p, q in pairs])
        fs = np.stack([np.array([[0, 0, sy * (q - p)], [0, 0, -sx * (q - p)], [-sy * (q - p), sx * (q - p), 0]], np.float32)
                       for p, q in pairs])
        dev = [torch.from_numpy(np.pad(d, ((0, 0), (0, 64 - d.shape[1])))).cuda() for _, d in f]
        row = {"pairs": len(pairs), "rows": [len(d) for _, d in f][:2]}
        row["blind_ms"] = median_ms(lambda: [ctx.descriptor_match(f[p][1], f[q][1], 10000, RATIO) for p, q in pairs])
        row["blind_device_ms"] = median_ms(lambda: [ctx.descriptor_match_device(dev[p], dev[q], 10000, RATIO) for p, q in pairs])
        if not blind_only:
            row["guided_H_ms"] = median_ms(lambda: ctx.descriptor_match_guided_pairs(f, pairs, hs, A.GUIDED_HOMOGRAPHY, RADIUS, 10000, RATIO))
            row["guided_F_ms"] = median_ms(lambda: ctx.descriptor_match_guided_pairs(f, pairs, fs, A.GUIDED_FUNDAMENTAL, RADIUS, 10000, RATIO))
            row["composite_ms"] = median_ms(lambda: ctx.match_features_homography_guided_pairs(f, pairs, RATIO, TRIALS, EPS, RADIUS, RATIO))

            def two_calls():
                base = ctx.match_features_homography_pairs(f, pairs, RATIO, TRIALS, EPS)
                found = [k for k, (_, h) in enumerate(base) if h is not None]
                if found:
                    ctx.descriptor_match_guided_pairs(f, [pairs[k] for k in found], np.stack([base[k][1] for k in found]),
                                                      A.GUIDED_HOMOGRAPHY, RADIUS, 10000, RATIO)
            row["two_calls_ms"] = median_ms(two_calls)
            row["homography_ms"] = median_ms(lambda: ctx.match_features_homography_pairs(f, pairs, RATIO, TRIALS, EPS))
            # what the lists hold
            A.random_seed(42, 69)
            base = ctx.match_features_homography_pairs(f, pairs, RATIO, TRIALS, EPS)
            A.random_seed(42, 69)
            comp = ctx.match_features_homography_guided_pairs(f, pairs, RATIO, TRIALS, EPS, RADIUS, RATIO)
            gf = ctx.descriptor_match_guided_pairs(f, pairs, fs, A.GUIDED_FUNDAMENTAL, RADIUS, 10000, RATIO)
            row["matches"] = {"blind": sum(len(ctx.descriptor_match(f[p][1], f[q][1], 10000, RATIO)) for p, q in pairs),
                              "homography": sum(len(x) for x, _ in base), "composite": sum(len(x) for x, _ in comp),
                              "guided_F": sum(len(x) for x in gf), "found": sum(h is not None for _, h in comp)}
        rows[name] = row
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="akaze-rust_amd directory of the build whose blind scan is the yardstick")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_guided.json"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("PKG", "WHAT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    here = os.path.join(ROOT, "akaze-rust_amd")
    if args.child:
        print(json.dumps(child(args.child[0], args.reps, args.child[1] == "blind", False)))
        return
    if args.trace:
        child(here, 1, False, True)
        return

    def run(pkg, what):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pkg, what, "--reps", str(args.reps)], check=True,
                             capture_output=True, text=True, timeout=500).stdout
        return json.loads(out.strip().splitlines()[-1])
    doc = {"tool": "tools/guided_match.py", "trials": TRIALS, "epsilon": EPS, "ratio": RATIO, "guided_radius": RADIUS,
           "reps": args.reps, "this_build": run(here, "all")}
    if args.baseline:
        doc["baseline_blind"] = run(args.baseline, "blind")
    ratios = {}
    for name, row in doc["this_build"].items():
        base = doc.get("baseline_blind", doc["this_build"])[name]
        blind, blind_dev = base["blind_ms"], base["blind_device_ms"]
        ratios[name] = {"guided_H_over_blind": round(row["guided_H_ms"] / blind, 3),
                        "guided_F_over_blind": round(row["guided_F_ms"] / blind, 3),
                        "guided_H_over_blind_device": round(row["guided_H_ms"] / blind_dev, 3),
                        "guided_F_over_blind_device": round(row["guided_F_ms"] / blind_dev, 3),
                        "blind_this_over_baseline": round(row["blind_ms"] / blind, 3),
                        "blind_device_this_over_baseline": round(row["blind_device_ms"] / blind_dev, 3),
                        "composite_over_two_calls": round(row["composite_ms"] / row["two_calls_ms"], 3)}
    doc["ratios"] = ratios
    import torch
    doc["device"] = torch.cuda.get_device_name(0)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
