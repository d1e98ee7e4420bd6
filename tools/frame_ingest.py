#!/usr/bin/env python3
"""Frame ingest (akz_luma_from_frames_device, akz_extract_device_frames, akz_extract_begin_device_frames) measured on the sizes a
user runs: 32 x 1920x1080 and 8 x 3840x2160, as RGB8 tight, RGB8 with a pitch of 3 w + 1, BGRA8 and planar RGB.

    timeout -k 10 900 python tools/frame_ingest.py [--rounds 15] [--out profiles/r26_frame_ingest.json]

(a) `kernel_vs_copy`   k_frame_luma against a device-to-device copy (torch's copy_ of a contiguous uint8 range, on the same stream), device events round an inner run of --inner launches, the two
                       forms alternating round by round, medians of --rounds after a warm-up.  `copy_2px` moves 2 w h n bytes (it
                       reads and writes what RGB8 -> luma reads and writes); `copy_same_traffic` moves half of the form's own
                       traffic (2.5 w h n for BGRA8).  ratio = kernel / copy_2px.
(b) `extract`          per call, host clock (the calls are synchronous), two alternations: extract_frames on RGB8 against
                       extract_features on luma frames that are ready (the added cost of the ingest), and against the torch flow a
                       caller had before ((t.float() @ weights).to(uint8), NOT bit-identical -- its keypoint counts are beside the
                       times --, then extract_features); `conversion_alone`: the torch expression and k_frame_luma by device events.
(c) `streamed`         begin / finish with three jobs in flight, ms per frame in steady state: the luma stream
                       (extract_begin) and the frames stream (extract_frames_begin), each with and without input_ready.
Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akaze-rust_amd", "python"))
import akaze_amd as A  # noqa: E402
import numpy as np  # noqa: E402

SIZES = [("32x1080p", 1920, 1080, 32), ("8x2160p", 3840, 2160, 8)]
FORMS = ["rgb8", "rgb8_pitch_3w+1", "bgra8", "rgb8_planar"]


def med(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=len(v))


_BASE = {}


def colour_frames(w, h, n, form, first=0):
    """(device view, layout, order, bytes read per pixel) of n synthetic colour frames in `form`"""
    import torch
    for i in range(first, first + n):
        if (w, h, i) not in _BASE:
            _BASE[(w, h, i)] = torch.from_numpy(A.synth_frame(w, h, i)).cuda()
    base = torch.stack([_BASE[(w, h, i)] for i in range(first, first + n)])
    r, g, b = base, base.flip(1), base.flip(2)  # three different pictures per frame
    if form == "rgb8":
        return torch.stack([r, g, b], dim=-1).contiguous(), "hwc", "rgb", 3
    if form == "rgb8_pitch_3w+1":
        buf = torch.zeros((n, h, 3 * w + 1), dtype=torch.uint8, device="cuda")
        view = buf[:, :, :3 * w].unflatten(2, (w, 3))
        view.copy_(torch.stack([r, g, b], dim=-1))
        return view, "hwc", "rgb", 3
    if form == "bgra8":
        return torch.stack([b, g, r, r], dim=-1).contiguous(), "hwc", "bgr", 4
    return torch.stack([r, g, b], dim=1).contiguous(), "chw", "rgb", 3


def events(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def kernel_vs_copy(ctx, rounds, inner):
    import torch
    out = {}
    for name, w, h, n in SIZES:
        px = w * h * n
        luma = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        csrc = torch.empty(5 * px // 2, dtype=torch.uint8, device="cuda").fill_(7)
        cdst = torch.empty_like(csrc)
        for form in FORMS:
            t, layout, order, bpp = colour_frames(w, h, n, form)
            legs = {"kernel": lambda: ctx.luma_from_frames(t, layout, order, out=luma),
                    "copy_2px": lambda: cdst[:2 * px].copy_(csrc[:2 * px]),
                    "copy_same_traffic": lambda: cdst[:(bpp + 1) * px // 2].copy_(csrc[:(bpp + 1) * px // 2])}
            ms = {k: [] for k in legs}
            for r in range(rounds + 2):
                for k, fn in legs.items():
                    v = events(fn, inner)
                    if r >= 2:
                        ms[k].append(v)
            row = {k: med(v) for k, v in ms.items()}
            row["ratio_kernel_to_copy_2px"] = row["kernel"]["median"] / row["copy_2px"]["median"]
            row["ratio_kernel_to_copy_same_traffic"] = row["kernel"]["median"] / row["copy_same_traffic"]["median"]
            row["kernel_GBps"] = (bpp + 1) * px / row["kernel"]["median"] / 1e6
            row["copy_2px_GBps"] = 4 * px / row["copy_2px"]["median"] / 1e6
            out[f"{name}/{form}"] = row
            del t
    return out


def extract_legs(ctx, rounds):
    import torch
    weights = torch.tensor([0.2126, 0.7152, 0.0722], dtype=torch.float32, device="cuda")
    out = {}
    for name, w, h, n in SIZES:
        t, layout, order, _ = colour_frames(w, h, n, "rgb8")
        luma = ctx.luma_from_frames(t)
        ctx.synchronize()

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            dt = (time.perf_counter() - t0) * 1e3
            kp = sum(r.counts(i)[1] for i in range(n))
            r.close()
            return dt, kp

        frames = lambda: ctx.extract_frames(t, keep_all_planes=False)
        torch_luma = lambda: (t.float() @ weights).to(torch.uint8)
        # two alternations of their own: a job's candidate capacity follows the job before it, and the torch flow's luma has other
        # keypoints, so a leg that follows it would not be the leg that follows its own kind
        pairs = {"against_ready_luma": {"extract_frames_rgb8": frames,
                                        "extract_features_ready_luma": lambda: ctx.extract_features(luma, keep_all_planes=False)},
                 "against_torch_flow": {"extract_frames_rgb8": frames,
                                        "torch_luma_then_extract": lambda: ctx.extract_features(torch_luma(), keep_all_planes=False)}}
        row = {}
        for pname, legs in pairs.items():
            ms, kps = {k: [] for k in legs}, {}
            for r in range(rounds + 2):
                for k, fn in legs.items():
                    dt, kps[k] = timed(fn)
                    if r >= 2:
                        ms[k].append(dt)
            row[pname] = {k: med(v) for k, v in ms.items()}
            row[pname]["keypoints"] = kps
        a, b = row["against_ready_luma"], row["against_torch_flow"]
        row["added_ms_over_ready_luma"] = a["extract_frames_rgb8"]["median"] - a["extract_features_ready_luma"]["median"]
        row["frames_over_torch_flow"] = b["extract_frames_rgb8"]["median"] / b["torch_luma_then_extract"]["median"]
        # the two conversions alone, device events: the torch expression against k_frame_luma
        conv = {"torch_luma_only": [], "k_frame_luma_only": []}
        for r in range(rounds + 2):
            for k, fn in (("torch_luma_only", torch_luma), ("k_frame_luma_only", lambda: ctx.luma_from_frames(t, out=luma))):
                v = events(fn, 2)
                if r >= 2:
                    conv[k].append(v)
        row["conversion_alone"] = {k: med(v) for k, v in conv.items()}
        out[name] = row
        del t, luma
    return out


def streamed(ctx, rounds, jobs=12):
    import torch
    out = {}
    for name, w, h, n in (("8x1080p", 1920, 1080, 8), ("2x2160p", 3840, 2160, 2)):
        ts = [colour_frames(w, h, n, "rgb8", first=k)[0] for k in range(3)]
        lumas = [ctx.luma_from_frames(t) for t in ts]
        ctx.synchronize()

        def stream(begin, src):
            torch.cuda.synchronize()
            flight = [begin(src[k % 3]) for k in range(2)]
            t0 = None
            for k in range(2, jobs + 3):
                flight.append(begin(src[k % 3]))
                flight.pop(0).finish().close()
                if k == 2:
                    t0 = time.perf_counter()  # steady state from here: `jobs` more finishes
            dt = (time.perf_counter() - t0) * 1e3
            for j in flight:
                j.finish().close()
            return dt / (jobs * n)

        legs = {"luma_stream": lambda: stream(lambda s: ctx.extract_begin(s, keep_all_planes=False), lumas),
                "luma_stream_input_ready": lambda: stream(lambda s: ctx.extract_begin(s, keep_all_planes=False, input_ready=True), lumas),
                "frames_stream": lambda: stream(lambda s: ctx.extract_frames_begin(s, keep_all_planes=False), ts),
                "frames_stream_input_ready": lambda: stream(lambda s: ctx.extract_frames_begin(s, keep_all_planes=False, input_ready=True), ts)}
        ms = {k: [] for k in legs}
        for r in range(rounds + 1):
            for k, fn in legs.items():
                v = fn()
                if r >= 1:
                    ms[k].append(v)
        out[name] = {k: med(v) for k, v in ms.items()}
        out[name]["unit"] = "ms per frame, three jobs in flight"
        del ts, lumas
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_frame_ingest.json"))
    ap.add_argument("--only", default="abc")
    args = ap.parse_args()
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    doc = dict(tool="tools/frame_ingest.py", device=torch.cuda.get_device_name(0), rounds=args.rounds, inner=args.inner,
               gpu_max_hw_queues=os.environ.get("GPU_MAX_HW_QUEUES"), unit="ms")
    if "a" in args.only:
        doc["kernel_vs_copy"] = kernel_vs_copy(ctx, args.rounds, args.inner)
    if "b" in args.only:
        doc["extract"] = extract_legs(ctx, args.rounds)
    if "c" in args.only:
        doc["streamed"] = streamed(ctx, args.rounds)
    ctx.close()
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
