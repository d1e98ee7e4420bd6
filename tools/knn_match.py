#!/usr/bin/env python3
"""k-nearest-neighbour matching (akz_descriptor_match_knn_device) against the top-2 scan it was modelled on
(akz_descriptor_match_device), on device-resident rows.

    timeout -k 10 900 python tools/knn_match.py [--reps 5] [--baseline PARENT/akaze-rust_amd] [--rounds 2] [--out FILE]
    python tools/knn_match.py --resources          (no GPU: the compiler's resource usage of the kernels, per list length K)

Shapes (uniformly random 61-byte rows, seeded; threshold 10000): one pair at the golden images' feature counts, 7 393 x 5 630;
11 000 x 11 000; 65 536 x 65 536.  Per shape these legs alternate rep by rep (medians of --reps after one warm-up, with
min / max), every leg one enqueue and a synchronise of the context's stream, results left on the device:
  `knn_k1`, `knn_k2`, `knn_k4`, `knn_k8`   akz_descriptor_match_knn_device (builds that have the call);
  `top2`                                   akz_descriptor_match_device at ratio 0.86: the existing scan with its ratio test.
--baseline: every measurement runs in a child process of its own, --rounds times this build and the other one in turn; `ratios`
holds this build's knn_k* over the OTHER build's top2 per shape, `existing_path` this build's top2 over the other's.
`claim`: the k-list costs the scan one compare per accumulator -- refuted if knn_k2 at 65 536 x 65 536 takes more than 1.5 times
the other build's top2.  Prints one JSON document (and writes it to --out)."""
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
if "--pkg" in sys.argv:  # a child of --baseline: the build under PKG (its library and its binding), set before the import
    PKG = os.path.abspath(sys.argv[sys.argv.index("--pkg") + 1])
    os.environ["AKAZE_HIP_LIB"] = os.path.join(PKG, "libakaze_hip.so")
sys.path.insert(0, os.path.join(PKG, "python"))
import akaze_amd as A  # noqa: E402
import numpy as np  # noqa: E402

SHAPES = [("golden pair 7393 x 5630", 7393, 5630), ("11000 x 11000", 11000, 11000), ("65536 x 65536", 65536, 65536)]
KS = (1, 2, 4, 8)
RATIO, CLAIM_SHAPE, CLAIM_LIMIT = 0.86, "65536 x 65536", 1.5
HAS_KNN = hasattr(A.Context, "descriptor_match_knn_device")


def resources():
    """the compiler's remarks (-Rpass-analysis=kernel-resource-usage) for csrc/akz_knn.hip -> one row per kernel instance"""
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero", "-Rpass-analysis=kernel-resource-usage",
           "--cuda-device-only", "-S", "-o", os.devnull, os.path.join(PKG, "csrc", "akz_knn.hip")]
    err = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, check=True, text=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", line)
        if not m:
            continue
        if m.group(1):
            name = re.search(r"k_knn_(fp4|merge)ILi(\d+)E", m.group(1))
            cur = {"kernel": f"k_knn_{name.group(1)}<{name.group(2)}>" if name else m.group(1)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    keep = ("kernel", "VGPRs", "AGPRs", "SGPRs", "ScratchSize", "Occupancy", "VGPRs Spill", "SGPRs Spill", "LDS Size")
    return [{k: r[k] for k in keep if k in r} for r in rows]


def shape_row(ctx, name, n0, n1, reps):
    import torch
    rng = np.random.default_rng(18 + n0)
    rows = []
    for n in (n0, n1):
        r = np.zeros((n, 64), np.uint8)
        r[:, :61] = rng.integers(0, 256, (n, 61), dtype=np.uint8)
        rows.append(torch.from_numpy(r).cuda())

    def top2():
        res = ctx.descriptor_match_device(rows[0], rows[1], 10000, RATIO)
        ctx.synchronize()
        return res

    def knn(k):
        def run():
            res = ctx.descriptor_match_knn_device(rows[0], rows[1], k, 10000)
            ctx.synchronize()
            return res
        return run

    legs = {"top2": top2}
    if HAS_KNN:
        legs.update({f"knn_k{k}": knn(k) for k in KS})
    t = {leg: [] for leg in legs}
    res = {leg: fn() for leg, fn in legs.items()}  # warm-up, and the results
    for _ in range(reps):
        for leg, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            t[leg].append((time.perf_counter() - t0) * 1e3)
    row = {"shape": name, "n0": n0, "n1": n1, "runs": reps, "device": torch.cuda.get_device_name(0), "top2_matches": int(res["top2"][1].item())}
    for leg in legs:
        row[leg + "_ms"] = round(statistics.median(t[leg]), 4)
        row[leg + "_ms_min_max"] = [round(min(t[leg]), 4), round(max(t[leg]), 4)]
        row[leg + "_tera_pairs_per_s"] = round(n0 * n1 / (statistics.median(t[leg]) * 1e-3) / 1e12, 3)
    if HAS_KNN:  # k = 1 names the row that the top-2 scan names wherever that one keeps the query
        out, cnt = res["top2"]
        m = out[:int(cnt.item())].cpu().numpy().view(A.MATCH_DTYPE).reshape(-1)
        first = res["knn_k1"][0].cpu().numpy().view(A.MATCH_DTYPE).reshape(n0)
        row["knn_k1_agrees_with_top2"] = bool(np.array_equal(first[m["index_0"].astype(np.int64)], m))
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def against_baseline(baseline, rounds, reps):
    """this build and the build under `baseline`, each measurement in a child process, in turn"""
    runs = {"this": [], "baseline": []}
    for _ in range(rounds):
        for who, pkg in (("this", PKG), ("baseline", baseline)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--reps", str(reps), "--rows"], check=True,
                                 stdout=subprocess.PIPE, timeout=400).stdout
            runs[who].append(json.loads(out))
    ratios, existing, claim = [], [], None
    for i, first in enumerate(runs["this"][0]):
        old = [r[i]["top2_ms"] for r in runs["baseline"]]
        own = [r[i]["top2_ms"] for r in runs["this"]]
        spread = max(max(old) - min(old), max(own) - min(own))
        existing.append({"shape": first["shape"], "top2_ms_this": own, "top2_ms_baseline": old,
                         "ratio": round(statistics.median(own) / statistics.median(old), 3), "spread_ms": round(spread, 4),
                         "within_spread": bool(abs(statistics.median(own) - statistics.median(old)) <= spread)})
        for k in KS:
            new = [r[i][f"knn_k{k}_ms"] for r in runs["this"]]
            rec = {"shape": first["shape"], "k": k, "knn_ms_this": new, "top2_ms_baseline": old,
                   "ratio": round(statistics.median(new) / statistics.median(old), 3)}
            ratios.append(rec)
            if k == 2 and first["shape"] == CLAIM_SHAPE:
                claim = {"statement": "the k-list costs the scan one compare per accumulator: knn_k2 <= 1.5 x the baseline's top2 at 65536 x 65536",
                         "ratio": rec["ratio"], "limit": CLAIM_LIMIT, "verdict": "met" if rec["ratio"] <= CLAIM_LIMIT else "refuted"}
    return {"claim": claim, "ratios": ratios, "existing_path": existing, "rows_this": runs["this"], "rows_baseline": runs["baseline"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true", help="the kernels' resource usage alone (no GPU)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--baseline", help="akaze-rust_amd directory of a build to compare against (the parent commit's)")
    ap.add_argument("--rounds", type=int, default=2, help="with --baseline: child processes per build")
    ap.add_argument("--pkg", help="(child) the akaze-rust_amd directory of the build to measure")
    ap.add_argument("--rows", action="store_true", help="(child) print the shapes' rows alone")
    args = ap.parse_args()
    if args.resources:
        print(json.dumps({"tool": "tools/knn_match.py --resources", "kernels": resources()}, indent=1))
        return
    if not args.baseline and not args.rows:
        base = None
        import torch
        ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
        rows = [shape_row(ctx, name, n0, n1, args.reps) for name, n0, n1 in SHAPES]
        ctx.close()
    elif args.rows:
        import torch
        ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
        print(json.dumps([shape_row(ctx, name, n0, n1, args.reps) for name, n0, n1 in SHAPES]))
        ctx.close()
        return
    else:  # (this process never opens the GPU: the children do)
        base = against_baseline(os.path.abspath(args.baseline), args.rounds, args.reps)
        rows = base["rows_this"][-1]
    doc = {"tool": "tools/knn_match.py", "device": rows[0]["device"], "ratio_of_the_top2_leg": RATIO, "threshold": 10000,
           "notes": ["uniformly random 61-byte rows; every leg is one enqueue and a synchronise of the stream, results stay on the device",
                     "top2 is akz_descriptor_match_device, the scan with the ratio test; with --baseline the figure of the OTHER build is the yardstick"],
           "shapes": rows}
    try:
        doc["kernels"] = resources()
    except (OSError, subprocess.CalledProcessError) as e:
        doc["kernels"] = f"not available here: {e}"
    if base is not None:
        doc.update(base)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
