#!/usr/bin/env python3
"""The keypoint budget (akz_keypoint_budget_sets) against its host statement (akz_keypoint_budget_host), what it costs next to the
extraction, what it saves downstream, and what the two modes keep.

    timeout -k 10 900 python tools/keypoint_budget.py [--reps 5] [--out FILE]
    python tools/keypoint_budget.py --resources        (no GPU: the compiler's resource usage of the kernels)
    python tools/keypoint_budget.py --quality          (no GPU calls beyond the one extraction: part (c) alone)

Keypoints are real ones: those of tests/golden/1.jpg and 2.jpg at a detector threshold lowered until an image gives 11 000 (the
synthetic frames are too sparse), cut to each shape's count by a seeded random subsample, which keeps the spatial clustering and the
response distribution.
(a) `shapes`: 1 x 11 000, 32 x 6 000, 240 x 2 000, max_keypoints 2 000 (240 x 2 000: 500).  Per shape and mode the sets call (median
    of --reps after a warm-up, min / max), its split into upload, kernels and download (events on the stream), the host statement on
    the same sets, one thread, once; and the device call as a share of `extraction_ms`: the extraction call of as many synthetic
    frames (one 4K frame; 32 x 1080p in one batch; 240 x 1080p as 7.5 such batches), on this build.
(b) `downstream`: match_features_seeded_pairs on the golden pair's full sets against the sets cut to 2 000 by limit_features.
(c) `quality` (CPU, reported, not asserted): for N = 500 and 1 000 per mode, the share of 64-pixel cells of the image that hold a kept
    keypoint, and the inliers that remove_outliers_seeded keeps of descriptor_match_cross_host on the cut pair.
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "akaze-rust_amd")
sys.path.insert(0, os.path.join(PKG, "python"))
import akaze_amd as A  # noqa: E402
import numpy as np  # noqa: E402

GOLDEN = [os.path.join(ROOT, "tests", "golden", n) for n in ("1.jpg", "2.jpg")]
SHAPES = [("1 x 11000", 1, 11000, 2000, "1 x 3840x2160"), ("32 x 6000", 32, 6000, 2000, "32 x 1920x1080"),
          ("240 x 2000", 240, 2000, 500, "240 x 1920x1080")]
MODES = (("spread", A.BUDGET_SPREAD), ("strongest", A.BUDGET_STRONGEST))
ROBUST = 0.9


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def resources():
    """the compiler's remarks (-Rpass-analysis=kernel-resource-usage) for csrc/akz_budget.hip -> one row per kernel"""
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero", "-Rpass-analysis=kernel-resource-usage",
           "--cuda-device-only", "-S", "-o", os.devnull, os.path.join(PKG, "csrc", "akz_budget.hip")]
    err = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, check=True, text=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: (?:[^ ]+ )?(?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", line)
        if not m:
            continue
        if m.group(1):
            name = re.search(r"(k_budget_[a-z]+)(?:ILb([01])E)?", m.group(1))
            cur = {"kernel": (name.group(1) + ("<rank>" if name.group(2) == "1" else "<radius>" if name.group(2) else "")) if name else m.group(1)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    keep = ("kernel", "VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "VGPRs Spill", "SGPRs Spill", "LDS Size")
    return [{k: r[k] for k in keep if k in r} for r in rows]


def golden_pools(ctx):
    """-> (the golden pair's (keypoints, descriptors) at the default threshold, per image a pool of >= 11 000 keypoints, its threshold)"""
    res = ctx.extract_features_files(GOLDEN, keep_all_planes=False)
    full = [(res.keypoints(i), res.descriptors(i)) for i in (0, 1)]
    for thr in (0.001, 0.0005, 0.00025, 0.0001, 0.00005, 0.00002):
        cfg = A.Config()
        cfg.detector_threshold = thr
        res = ctx.extract_features_files(GOLDEN, cfg, keep_all_planes=False)
        pools = [res.keypoints(i) for i in (0, 1)]
        if min(len(p) for p in pools) >= 11000:
            break
    return full, pools, thr


def subsample(pool, n, seed):
    idx = np.sort(np.random.default_rng(seed).permutation(len(pool))[:n])  # (the detector's order is kept)
    return np.ascontiguousarray(pool[idx])


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 4), [round(min(t), 4), round(max(t), 4)]


def extraction_ms(ctx, w, h, n, reps):
    """the extraction call of n synthetic w x h frames in one batch (uint8, on the device), keypoints per frame"""
    import torch
    frames = torch.from_numpy(np.stack([A.synth_frame(w, h, i) for i in range(n)])).cuda()
    res = ctx.extract_features(frames, keep_all_planes=False)
    kps = [res.counts(i)[1] for i in range(n)]
    ms, _ = timed(lambda: ctx.extract_features(frames, keep_all_planes=False), reps)
    return ms, int(statistics.median(kps))


def shape_rows(ctx, pools, reps):
    ext = {}
    ext["1 x 3840x2160"], kp4k = extraction_ms(ctx, 3840, 2160, 1, reps)
    ext["32 x 1920x1080"], kp1080 = extraction_ms(ctx, 1920, 1080, 32, reps)
    ext["240 x 1920x1080"] = round(7.5 * ext["32 x 1920x1080"], 4)
    log("extraction", ext, kp4k, kp1080)
    rows = []
    for name, n_sets, n, keep, frames in SHAPES:
        sets = [subsample(pools[s % 2], n, 1000 * n_sets + s) for s in range(n_sets)]
        row = {"shape": name, "sets": n_sets, "keypoints_per_set": n, "max_keypoints": keep, "extraction_frames": frames,
               "extraction_ms": ext[frames]}
        for mname, mode in MODES:
            ctx.debug_keypoint_budget_split(True)
            ms, mm = timed(lambda: ctx.keypoint_budget_sets(sets, keep, mode, ROBUST), reps)
            split = ctx.debug_keypoint_budget_split(False)
            got = ctx.keypoint_budget_sets(sets, keep, mode, ROBUST)
            t0 = time.perf_counter()
            exp = [A.keypoint_budget_host(k, keep, mode, ROBUST) for k in sets]
            host_ms = (time.perf_counter() - t0) * 1e3
            same = all(g[0].tobytes() == e[0].tobytes() and (g[1] is None or g[1].tobytes() == e[1].tobytes()) for g, e in zip(got, exp))
            row[mname] = {"device_ms": ms, "device_ms_min_max": mm, "upload_kernels_download_ms": [round(v, 4) for v in split],
                          "host_statement_ms": round(host_ms, 3), "host_over_device": round(host_ms / ms, 2),
                          "share_of_extraction": round(ms / ext[frames], 4), "equals_host_statement": bool(same)}
            log(name, mname, row[mname])
        rows.append(row)
    return rows, {"synthetic_keypoints_per_frame": {"3840x2160": kp4k, "1920x1080": kp1080}}


def downstream(ctx, full, reps):
    opt = A.RansacOptions()
    row = {"sets": [len(k) for k, _ in full], "budget": 2000}
    ms, mm = timed(lambda: ctx.match_features_seeded_pairs(full, [(0, 1)], opt), reps)
    row["full"] = {"seeded_pairs_ms": ms, "min_max": mm, "kept": len(ctx.match_features_seeded_pairs(full, [(0, 1)], opt)[0][0])}
    for mname, mode in MODES:
        cut_ms, _ = timed(lambda: ctx.keypoint_budget_sets(full, 2000, mode, ROBUST), reps)
        cut = [A.limit_features(k, d, 2000, mode, ROBUST, ctx=ctx)[:2] for k, d in full]
        ms, mm = timed(lambda: ctx.match_features_seeded_pairs(cut, [(0, 1)], opt), reps)
        row[mname] = {"budget_call_ms": cut_ms, "seeded_pairs_ms": ms, "min_max": mm,
                      "kept": len(ctx.match_features_seeded_pairs(cut, [(0, 1)], opt)[0][0])}
    log("downstream", row)
    return row


def quality(full, shape):
    """(c), on the CPU: cell coverage and inliers per mode and budget"""
    h, w = shape
    cells = ((w + 63) // 64) * ((h + 63) // 64)
    rows = []
    for n in (500, 1000):
        for mname, mode in MODES:
            cut, cover = [], []
            for k, d in full:
                idx = A.keypoint_budget_host(k, n, mode, ROBUST)[0].astype(np.int64)
                cut.append((k[idx], d[idx]))
                cover.append(len(set(zip((k["x"][idx] // 64).astype(int), (k["y"][idx] // 64).astype(int)))) / cells)
            raw = A.descriptor_match_cross_host(cut[0][1], cut[1][1], 10000, 0.86)
            kept = A.remove_outliers_seeded(cut[0][0], cut[1][0], raw, A.RansacOptions())[0] if len(raw) else raw
            rows.append({"budget": n, "mode": mname, "cells_covered": [round(c, 4) for c in cover], "cross_checked_matches": len(raw),
                         "ransac_inliers": len(kept)})
            log("quality", rows[-1])
    return {"cell_px": 64, "cells": cells, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true", help="the kernels' resource usage alone (no GPU)")
    ap.add_argument("--quality", action="store_true", help="part (c) alone")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    args = ap.parse_args()
    if args.resources:
        print(json.dumps({"tool": "tools/keypoint_budget.py --resources", "kernels": resources()}, indent=1))
        return
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    full, pools, thr = golden_pools(ctx)
    doc = {"tool": "tools/keypoint_budget.py", "device": torch.cuda.get_device_name(0), "robust": ROBUST,
           "tiles": dict(zip(("query_tile", "train_stage"), A.keypoint_budget_tiles())),
           "keypoint_pools": {"images": ["1.jpg", "2.jpg"], "detector_threshold": thr, "keypoints": [len(p) for p in pools]}}
    if not args.quality:
        doc["shapes"], extra = shape_rows(ctx, pools, args.reps)
        doc.update(extra)
        doc["downstream"] = downstream(ctx, full, args.reps)
    ctx.close()
    doc["quality"] = quality(full, A.load_image_luma(GOLDEN[0]).shape)
    try:
        doc["kernels"] = resources()
    except (OSError, subprocess.CalledProcessError) as e:
        doc["kernels"] = f"not available here: {e}"
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
