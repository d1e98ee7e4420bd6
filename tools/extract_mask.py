#!/usr/bin/env python3
"""The detection mask (akz_extract_device_frames_masked) measured on the sizes a user runs: 32 x 1920x1080 RGB frames per call and a
lone 1920x1080 RGB frame per call, synchronous calls.

    timeout -k 10 900 python tools/extract_mask.py [--parent-tree DIR] [--steps 20] [--out profiles/r27_extract_mask.json]

Legs, per workload:
  parent        extract_frames of the parent commit (--parent-tree: a checkout of it with akaze-rust_amd built; its binding and its
                library, in a process of their own; left out when the option is not given)
  unmasked      extract_frames, this build
  ones          ... with an all-ones mask
  left_half     ... with a mask that keeps the left half
  tenth         ... with a mask that keeps the left tenth
Protocol, as bench.py --full: a warm-up, then five timed regions of --steps calls each, host clock round a region (the calls are
synchronous); a leg's figure is its MEDIAN region in ms per call, all five are kept.  The legs of this build alternate region by
region.  The filter kernel's own time comes from the kernel rows (k_mask_candidates, HIP events, full stage profiling) of
--steps further calls per masked leg, outside the timed regions.  Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.environ.get("EXTRACT_MASK_TREE") or ROOT, "akaze-rust_amd", "python"))  # (the parent leg: that tree's binding)

WORKLOADS = [("32x1080p", 1920, 1080, 32), ("1x1080p", 1920, 1080, 1)]
REGIONS = 5
MASKS = ("ones", "left_half", "tenth")


def frames(A, w, h, n):
    import torch
    base = torch.stack([torch.from_numpy(A.synth_frame(w, h, i)).cuda() for i in range(n)])
    return torch.stack([base, base.flip(1), base.flip(2)], dim=-1).contiguous()  # three different pictures per frame


def make_mask(name, w, h):
    import torch
    m = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    m[:, :{"ones": w, "left_half": w // 2, "tenth": w // 10}[name]] = 255
    return m


def region(ctx, t, mask, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = ctx.extract_frames(t, keep_all_planes=False, mask=mask) if mask is not None else ctx.extract_frames(t, keep_all_planes=False)
        kp = sum(r.counts(i)[1] for i in range(r.num_images))
        r.close()
    return (time.perf_counter() - t0) * 1e3 / steps, kp


def summary(ms, kp):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), regions=ms, keypoints_per_call=kp, unit="ms per call")


def run_legs(legs, steps):
    """legs: name -> mask or None; returns name -> summary.  Every leg is warmed, then the regions alternate between the legs."""
    import akaze_amd as A
    import torch
    out = {}
    for wname, w, h, n in WORKLOADS:
        ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
        t = frames(A, w, h, n)
        masks = {k: (make_mask(k, w, h) if k in MASKS else None) for k in legs}
        for k in legs:
            region(ctx, t, masks[k], 3)
        ms, kps = {k: [] for k in legs}, {}
        for _ in range(REGIONS):
            for k in legs:
                v, kps[k] = region(ctx, t, masks[k], steps)
                ms[k].append(v)
        row = {k: summary(ms[k], kps[k]) for k in legs}
        # the filter kernel alone: its kernel row under full stage profiling
        ctx.set_profiling(1)
        for k in legs:
            if masks[k] is None or not hasattr(A, "KR_MASK_CANDIDATES"):
                continue
            ctx.kernel_rows(reset=True)
            region(ctx, t, masks[k], steps)
            rows = [r for r in ctx.kernel_rows(reset=True) if r["kind"] == A.KR_MASK_CANDIDATES]
            counts = ctx.debug_mask_counts()
            row[k]["k_mask_candidates"] = dict(launches=sum(r["launches"] for r in rows), ms_per_launch=sum(r["ms"] for r in rows) / max(1, sum(r["launches"] for r in rows)),
                                               list_capacity=rows[0]["px"] // max(1, rows[0]["launches"]) if rows else 0,
                                               candidates_before=counts["unfiltered"], candidates_kept=counts["kept"], passes_redone=counts["redone"])
        ctx.set_profiling(0)
        out[wname] = row
        ctx.close()
        del t, masks
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with akaze-rust_amd built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_extract_mask.json"))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)  # "parent": this process IS the parent leg (EXTRACT_MASK_TREE is set)
    args = ap.parse_args()
    if args.leg == "parent":
        print(json.dumps(run_legs(["parent"], args.steps)))
        return
    import torch
    doc = dict(tool="tools/extract_mask.py", device=torch.cuda.get_device_name(0), steps=args.steps, regions=REGIONS,
               gpu_max_hw_queues=os.environ.get("GPU_MAX_HW_QUEUES"))
    parent = None
    if args.parent_tree:
        env = dict(os.environ, EXTRACT_MASK_TREE=os.path.abspath(args.parent_tree))
        env.pop("AKAZE_HIP_LIB", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "parent", "--steps", str(args.steps)], env=env,
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise SystemExit("the parent leg failed:\n" + p.stderr[-2000:])
        parent = json.loads(p.stdout.strip().splitlines()[-1])
    mine = run_legs(["unmasked"] + list(MASKS), args.steps)
    doc["workloads"] = {w: dict(**(parent[w] if parent else {}), **mine[w]) for w in mine}
    for w, row in doc["workloads"].items():
        u = row["unmasked"]["median"]
        row["delta_ms_vs_unmasked"] = {k: row[k]["median"] - u for k in row if k not in ("unmasked",) and isinstance(row[k], dict) and "median" in row[k]}
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
