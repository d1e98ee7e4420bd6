#!/usr/bin/env python3
"""File-based extraction with JPEG reconstruction on the device, against the host-decode path it replaces.

    timeout -k 10 900 python tools/jpeg_ingest.py [--reps 7] [--out FILE]               # timings (one GPU process)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/jpeg_ingest.py --trace   # kernel stats

On tests/golden/1.jpg, 2.jpg and match_image.jpg, variants alternated rep by rep (A/B/A/B...), medians of --reps runs after
two warm-ups, all in one process on one context:
  * extract: akz_image_load_luma + akz_extract_gray_u8 (the old file path) against akz_extract_features_file;
  * decode: akz_image_load_luma (host) against akz_image_load_luma_device;
  * batch: akz_extract_features_files over 8 and 32 paths (1.jpg / 2.jpg alternating) at 1, 4 and 16 host threads, against a
    per-file loop of the old path, as files per second;
  * device rows: the spans of the coefficient upload, k_jpeg_idct and k_jpeg_luma (akz_debug_kernel_rows, profiling on,
    one extra run per file), with the bytes each must move -- the IDCT reads 2 B per coefficient and writes 1 B per
    sample, the luma pass reads the component samples it needs and writes 1 B per pixel -- and the extraction's own
    device stages of the same run beside them.
Prints one JSON document (and writes it to --out if given).  --trace: one pass of every call, nothing timed (for rocprofv3)."""
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
import akaze_amd as A  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ["1.jpg", "2.jpg", "match_image.jpg"]


def ms_of(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def alternate(variants, reps, warm=2):
    """variants: {name: fn}; A/B alternated; {name: median ms, name_min, name_max}."""
    for _ in range(warm):
        for fn in variants.values():
            fn()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(ms_of(fn))
    out = {}
    for k, t in times.items():
        out[k] = {"ms": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3), "runs": len(t)}
    return out


def sof(path):
    """(w, h, [(h, v)]) from the frame header."""
    d = open(path, "rb").read()
    p = 2
    while p + 4 <= len(d):
        if d[p] != 0xFF or d[p + 1] in (0x00, 0xFF):
            p += 1
            continue
        m, ln = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        if m in (0xC0, 0xC1, 0xC2):
            b = d[p + 4:]
            return (b[3] << 8) | b[4], (b[1] << 8) | b[2], [(b[7 + 3 * i] >> 4, b[7 + 3 * i] & 15) for i in range(b[5])]
        p += 2 + ln
    raise ValueError(path)


def luma_read_bytes(w, h, f):
    """Bytes k_jpeg_luma must read: every sample of the upsampled components that the frame covers."""
    hmax, vmax = max(x[0] for x in f), max(x[1] for x in f)
    return sum(-(-w * ch // hmax) * -(-h * cv // vmax) for ch, cv in f)


def old_path(ctx, path):
    L = A.lib()
    w, h, px = C.c_uint32(), C.c_uint32(), C.c_void_p()
    A._check(L.akz_image_load_luma(os.fsencode(path), C.byref(w), C.byref(h), C.byref(px)))
    res = C.c_void_p()
    cfg = A.Config()
    st = L.akz_extract_gray_u8(ctx._h, px, w.value, h.value, C.byref(cfg), 0, C.byref(res))
    L.akz_image_free(px)
    A._check(st)
    L.akz_result_free(res)


def new_path(ctx, path):
    L = A.lib()
    res = C.c_void_p()
    cfg = A.Config()
    A._check(L.akz_extract_features_file(ctx._h, os.fsencode(path), C.byref(cfg), 0, C.byref(res)))
    L.akz_result_free(res)


def batch(ctx, paths):
    L = A.lib()
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    res = C.c_void_p()
    cfg = A.Config()
    A._check(L.akz_extract_features_files(ctx._h, arr, len(paths), C.byref(cfg), 0, C.byref(res)))
    L.akz_result_free(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import torch
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    paths = {n: os.path.join(GOLDEN, n) for n in FILES}
    pair = [paths["1.jpg"], paths["2.jpg"]]
    if a.trace:
        for p in paths.values():
            old_path(ctx, p)
            new_path(ctx, p)
            ctx.load_luma_device(p)
        batch(ctx, pair * 4)
        torch.cuda.synchronize()
        return
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "host_cpus_usable": len(os.sched_getaffinity(0)),
           "files": {}, "batch": {}}
    dev_bufs = {}
    for n, p in paths.items():
        w, h, f = sof(p)
        dev_bufs[n] = torch.empty(w * h, dtype=torch.uint8, device="cuda")
        buf = dev_bufs[n]

        def load_dev(p=p, buf=buf):
            w_, h_ = C.c_uint32(), C.c_uint32()
            A._check(A.lib().akz_image_load_luma_device(ctx._h, os.fsencode(p), C.c_void_p(buf.data_ptr()), buf.numel(),
                                                        C.byref(w_), C.byref(h_)))

        ex = alternate({"old_path": lambda p=p: old_path(ctx, p), "extract_features_file": lambda p=p: new_path(ctx, p)}, a.reps)
        de = alternate({"image_load_luma": lambda p=p: A.load_image_luma(p), "image_load_luma_device": load_dev}, a.reps)
        # device rows of one profiled extract_features_file
        ctx.set_profiling(1)
        ctx.kernel_rows(reset=True)
        ctx.get_profile(reset=True)
        new_path(ctx, p)
        rows = ctx.kernel_rows(reset=True)
        prof = ctx.get_profile(reset=True)
        ctx.set_profiling(0)
        coefs = sum(-(-w // (8 * max(x[0] for x in f))) * x[0] * -(-h // (8 * max(x[1] for x in f))) * x[1] * 64 for x in f)
        jr = {}
        for r in rows:
            if r["kind"] not in (6, 7, 8) or not r["launches"]:
                continue
            if r["kind"] == 6:
                moved = 3 * r["px"]
            elif r["kind"] == 7:
                moved = luma_read_bytes(w, h, f) + w * h
            else:
                moved = r["px"]
            jr[r["kernel"]] = {"ms": round(r["ms"], 4), "bytes": int(moved), "gb_s": round(moved / max(r["ms"], 1e-9) / 1e6, 1)}
        extraction_device_ms = sum(prof[k] for k in A.STAGES[:6])
        kern_ms = sum(v["ms"] for k, v in jr.items() if k.startswith("k_jpeg"))
        doc["files"][n] = {
            "w": w, "h": h, "sampling": f, "coefficients": coefs,
            "extract": ex, "speedup_extract": round(ex["old_path"]["ms"] / ex["extract_features_file"]["ms"], 2),
            "decode": de, "speedup_decode": round(de["image_load_luma"]["ms"] / de["image_load_luma_device"]["ms"], 2),
            "device_rows": jr, "jpeg_kernels_ms": round(kern_ms, 4),
            "extraction_device_stages_ms": round(extraction_device_ms, 4),
            "jpeg_kernels_share_of_extraction": round(kern_ms / max(extraction_device_ms, 1e-9), 4),
            "copy_share_of_jpeg_device_time": round(jr.get("jpeg_coef_h2d", {"ms": 0})["ms"] / max(sum(v["ms"] for v in jr.values()), 1e-9), 4),
        }
    for nfiles in (8, 32):
        ps = (pair * nfiles)[:nfiles]
        variants = {"per_file_old_path": lambda ps=ps: [old_path(ctx, p) for p in ps]}
        for t in (1, 4, 16):
            def run(ps=ps, t=t):
                ctx.set_host_threads(t)
                batch(ctx, ps)
            variants[f"files_threads{t}"] = run
        r = alternate(variants, max(3, a.reps // 2), warm=1)
        ctx.set_host_threads(0)
        for k, v in r.items():
            v["files_per_s"] = round(nfiles / v["ms"] * 1e3, 2)
        r["speedup_threads16_vs_loop"] = round(r["files_threads16"]["files_per_s"] / r["per_file_old_path"]["files_per_s"], 2)
        doc["batch"][str(nfiles)] = r
    ctx.close()
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
