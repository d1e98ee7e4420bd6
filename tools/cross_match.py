#!/usr/bin/env python3
"""Cross-checked matching (akz_descriptor_match_cross_device, akz_match_features_seeded_cross_pairs) against what a caller did
before it existed, on the workloads of tools/seeded_ransac.py.

    timeout -k 10 1100 python tools/cross_match.py [--reps 5] [--baseline OTHER/akaze-rust_amd] [--rounds 2] [--out FILE]
    python tools/cross_match.py --host-statement      (no GPU: the CPU figures of CHANGELOG round 16, see host_statement)

Workloads, from synth_frame features of one scene with shifts: a lone 1080p pair and the exhaustive ordered pairs of 8 and 16
frames at 1920x1080 (56 and 240 pairs), ratio 0.86.  Per workload these legs alternate rep by rep (medians of --reps after one
warm-up, with min / max), every leg ending with its results on the host:
  `two_scans_host_intersect`  per pair two akz_descriptor_match_device calls (the sets exchanged), both lists downloaded, the
                              intersection in numpy -- the flow of a caller without the cross-check;
  `cross_device`              per pair akz_descriptor_match_cross_device and ONE download (builds that have the call);
  `match_device`              per pair akz_descriptor_match_device and its download: the existing one-directional path;
  `seeded`, `seeded_cross`    akz_match_features_seeded_pairs over the workload's pairs, fundamental matrix, 1 000 trials, epsilon
                              3.0, confidence 0.99, without and with cross_check (the latter on builds that have it);
  `host_draws`                akz_match_features_fundamental_pairs, the call that draws on the calling thread.
Beside the times: the list lengths with and without the cross-check, trials_run of the two seeded legs, and, from timed runs of
their own, the akz_debug_match_pairs_split of the two seeded legs (the filter launch lies in `scans`).
`price_of_the_option`: seeded_cross over seeded of this build, per workload.
--baseline: every measurement runs in a child process of its own, --rounds times this build and the other one in turn;
`claim_1` holds this build's cross_device against the OTHER build's two_scans_host_intersect with the spread between that leg's
rounds, `existing_paths` the ratio this / other of seeded, host_draws and match_device with whether they agree within 2 % or
within the rounds' own spread.  Prints one JSON document (and writes it to --out)."""
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
import numpy as np  # noqa: E402

TRIALS, RATIO, EPS = 1000, 0.86, 3.0
SPLIT = ["uploads", "scans", "host_draws", "trials", "pick_filter", "readback"]
HAS_CROSS = hasattr(A.Context, "descriptor_match_cross_device")


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


def records(out, cnt):
    n = int(cnt.item())  # (a device synchronise)
    return out[:n].cpu().numpy().view(A.MATCH_DTYPE).reshape(-1)


def workload(ctx, name, feats, pairs, reps):
    import torch
    rows = []
    for _, d in feats:
        r = np.zeros((len(d), 64), np.uint8)
        r[:, :d.shape[1]] = d
        rows.append(torch.from_numpy(r).cuda())

    def two_scans():
        out = []
        for a, b in pairs:
            fo, fc = ctx.descriptor_match_device(rows[a], rows[b], 10000, RATIO)
            f = records(fo, fc)
            ro, rc = ctx.descriptor_match_device(rows[b], rows[a], 10000, RATIO)
            r = records(ro, rc)
            back = np.full(len(rows[b]), -1, np.int64)
            back[r["index_0"].astype(np.int64)] = r["index_1"].astype(np.int64)
            out.append(f[back[f["index_1"].astype(np.int64)] == f["index_0"].astype(np.int64)])
        return out

    def cross_device():
        return [records(*ctx.descriptor_match_cross_device(rows[a], rows[b], 10000, RATIO)) for a, b in pairs]

    def match_device():
        return [records(*ctx.descriptor_match_device(rows[a], rows[b], 10000, RATIO)) for a, b in pairs]

    opt = A.RansacOptions(model_kind=A.GUIDED_FUNDAMENTAL, lowes_ratio=RATIO, max_trials=TRIALS, epsilon_inliers=EPS, confidence=0.99)
    legs = {"two_scans_host_intersect": two_scans, "match_device": match_device,
            "seeded": lambda: ctx.match_features_seeded_pairs(feats, pairs, opt),
            "host_draws": lambda: ctx.match_features_fundamental_pairs(feats, pairs, RATIO, TRIALS, EPS)}
    if HAS_CROSS:
        legs["cross_device"] = cross_device
        legs["seeded_cross"] = lambda: ctx.match_features_seeded_pairs(feats, pairs, opt, cross_check=True)
    res = {leg: timed(fn)[1] for leg, fn in legs.items()}  # warm-up, and the results
    t = {leg: [] for leg in legs}
    for _ in range(reps):
        for leg, fn in legs.items():
            t[leg].append(timed(fn)[0])
    seeded_legs = [leg for leg in ("seeded", "seeded_cross") if leg in legs]
    split = {leg: [] for leg in seeded_legs}
    A.lib().akz_debug_match_pairs_split(ctx._h, 1, None)
    ms = (C.c_double * 6)()
    for _ in range(reps):
        for leg in seeded_legs:
            timed(legs[leg])
            A.lib().akz_debug_match_pairs_split(ctx._h, 1, ms)
            split[leg].append(list(ms))
    A.lib().akz_debug_match_pairs_split(ctx._h, 0, None)
    row = {"workload": name, "pairs": len(pairs), "runs": reps,
           "forward_matches_per_pair_median": statistics.median(len(m) for m in res["match_device"]),
           "cross_matches_per_pair_median": statistics.median(len(m) for m in res["two_scans_host_intersect"])}
    if HAS_CROSS:
        row["cross_device_equals_host_intersection"] = all(np.array_equal(x, y) for x, y in zip(res["cross_device"], res["two_scans_host_intersect"]))
    for leg in legs:
        row[leg + "_ms"] = round(statistics.median(t[leg]), 3)
        row[leg + "_ms_min_max"] = [round(min(t[leg]), 3), round(max(t[leg]), 3)]
    for leg in seeded_legs:
        runs = [r[3] for r in res[leg] if r[3]] or [0]
        row[leg + "_trials_run_min_median_max"] = [min(runs), statistics.median(runs), max(runs)]
        row[leg + "_kept_median"] = statistics.median(len(r[0]) for r in res[leg])
        row[leg + "_found"] = sum(r[1] is not None for r in res[leg])
        row[leg + "_split_ms"] = {key: round(statistics.median(s[i] for s in split[leg]), 3) for i, key in enumerate(SPLIT)}
    if HAS_CROSS:
        row["cross_device_over_two_scans"] = round(row["cross_device_ms"] / row["two_scans_host_intersect_ms"], 3)
        row["seeded_cross_over_seeded"] = round(row["seeded_cross_ms"] / row["seeded_ms"], 3)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def against_baseline(baseline, rounds, reps):
    """this build and the build under `baseline`, each measurement in a child process, in turn"""
    runs = {"this": [], "baseline": []}
    for _ in range(rounds):
        for who, pkg in (("this", PKG), ("baseline", baseline)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--reps", str(reps), "--rows"], check=True,
                                 stdout=subprocess.PIPE, timeout=900).stdout
            runs[who].append(json.loads(out))
    claim, existing = [], []
    for i, first in enumerate(runs["this"][0]):
        new = [r[i]["cross_device_ms"] for r in runs["this"]]
        old = [r[i]["two_scans_host_intersect_ms"] for r in runs["baseline"]]
        spread = max(old) - min(old)
        claim.append({"workload": first["workload"], "cross_device_ms_this": new, "two_scans_host_intersect_ms_baseline": old,
                      "ratio": round(statistics.median(new) / statistics.median(old), 3), "baseline_spread_ms": round(spread, 3),
                      "no_slower_within_baseline_spread": bool(statistics.median(new) <= statistics.median(old) + spread)})
        for leg in ("seeded", "host_draws", "match_device"):
            ms = {who: [r[i][leg + "_ms"] for r in runs[who]] for who in runs}
            med = {who: statistics.median(v) for who, v in ms.items()}
            spread = max(max(v) - min(v) for v in ms.values())
            existing.append({"workload": first["workload"], "leg": leg, "this_ms": ms["this"], "baseline_ms": ms["baseline"],
                             "ratio": round(med["this"] / med["baseline"], 3), "spread_ms": round(spread, 3),
                             "within_spread": bool(abs(med["this"] - med["baseline"]) <= spread),
                             "within_2_percent": bool(med["this"] <= 1.02 * med["baseline"])})
    return {"claim_1": claim, "existing_paths": existing, "rows_this": runs["this"], "rows_baseline": runs["baseline"]}


def host_statement(streams=8):
    """--host-statement (no GPU): what the cross-check does to the list and to the seeded RANSAC (kind 3, 2 px, confidence 0.99, at
    most 1 000 trials, streams 0 .. streams - 1), with akz_descriptor_match_cross_host and akz_remove_outliers_seeded, on the oracle's
    features of tests/golden/1.jpg / 2.jpg in both orders and on two_view_scene cases with planted descriptors and rivals
    (tests/test_cross_match_host.py: cross_scene) -> one row per case"""
    for d in ("tests", "oracle"):
        sys.path.insert(0, os.path.join(ROOT, d))
    import akaze_ref
    from test_cross_match_host import cross_scene
    opt = A.RansacOptions(model_kind=A.RANSAC_FUNDAMENTAL_NORMALISED, max_trials=TRIALS, confidence=0.99, epsilon_inliers=2.0)

    def case(name, fa, fb):
        lists = {"forward": akaze_ref.descriptor_match(fa[1], fb[1], 10000, RATIO), "cross": A.descriptor_match_cross_host(fa[1], fb[1], 10000, RATIO)}
        row = {"case": name, "n0": len(fa[1]), "n1": len(fb[1])}
        for tag, lst in lists.items():
            res = [A.remove_outliers_seeded(fa[0], fb[0], lst, opt, stream=s) for s in range(streams)]
            kept, runs = [len(r[0]) for r in res], [r[3] for r in res]
            row.update({tag: len(lst), tag + "_kept_median": statistics.median(kept),
                        tag + "_share_kept_median": round(statistics.median(kept) / max(1, len(lst)), 3),
                        tag + "_trials_run_min_median_max": [min(runs), statistics.median(runs), max(runs)],
                        tag + "_found": sum(r[1] is not None for r in res)})
        return row

    golden = [akaze_ref.extract(A.load_image_luma(os.path.join(ROOT, "tests", "golden", n))) for n in ("1.jpg", "2.jpg")]
    g = [(r.keypoints(), r.descriptors()) for r in golden]
    rows = [case("golden 1.jpg / 2.jpg", g[0], g[1]), case("golden 2.jpg / 1.jpg", g[1], g[0])]
    for n, seed in ((257, 757), (1000, 758), (1000, 759)):
        rows.append(case(f"two_view_scene({seed}, {n}) + {n // 4} rivals at 30 bits", *cross_scene(A, "F", n, seed)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-statement", action="store_true", help="the CPU measurement alone (no GPU): list lengths, share kept, trials_run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--baseline", help="akaze-rust_amd directory of a build to compare against")
    ap.add_argument("--rounds", type=int, default=2, help="with --baseline: child processes per build")
    ap.add_argument("--pkg", help="(child) the akaze-rust_amd directory of the build to measure")
    ap.add_argument("--rows", action="store_true", help="(child) print the workloads' rows alone")
    args = ap.parse_args()
    if args.host_statement:
        print(json.dumps({"tool": "tools/cross_match.py --host-statement", "cases": host_statement()}, indent=1))
        return
    base = against_baseline(os.path.abspath(args.baseline), args.rounds, args.reps) if args.baseline else None  # (before this process opens the GPU)
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    f1080 = features(ctx, 1920, 1080, 16)
    jobs = [("1 pair 1080p", f1080[:2], [(0, 1)]),
            ("exhaustive 8 x 1080p", f1080[:8], [(a, b) for a in range(8) for b in range(8) if a != b]),
            ("exhaustive 16 x 1080p", f1080[:16], [(a, b) for a in range(16) for b in range(16) if a != b])]
    rows = [workload(ctx, name, feats, pairs, args.reps) for name, feats, pairs in jobs]
    if args.rows:
        print(json.dumps(rows))
        ctx.close()
        return
    doc = {"tool": "tools/cross_match.py", "device": torch.cuda.get_device_name(0), "trials": TRIALS, "ratio": RATIO, "epsilon": EPS,
           "notes": ["every leg ends with its lists on the host; two_scans_host_intersect is the flow of a caller without the cross-check",
                     "seeded / seeded_cross: fundamental matrix (the reference's trial model), confidence 0.99, as profiles/r14_seeded_ransac.json"],
           "workloads": rows,
           "price_of_the_option": [{"workload": r["workload"], "seeded_ms": r["seeded_ms"], "seeded_cross_ms": r["seeded_cross_ms"],
                                    "ratio": r["seeded_cross_over_seeded"]} for r in rows if HAS_CROSS]}
    if base is not None:
        doc.update(base)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
