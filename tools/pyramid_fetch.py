#!/usr/bin/env python3
"""Download of a whole EvolutionStep pyramid (Vec<EvolutionStep>, 10 planes per level) to host memory: akz_fetch_pyramid
into pageable and into pinned memory against the per-plane akz_fetch_plane loop (what the Rust shim does), with the
measured device-to-host ceiling of the same byte count (one akz_memcpy_d2h: hipMemcpyAsync + synchronise) beside it.

    timeout -k 10 600 python tools/pyramid_fetch.py [--reps 10] [--out FILE]

One synthetic u8 frame per shape, every plane of every level, all planes kept and lean (the four planes akz_fetch_pyramid
recomputes once per level, akz_fetch_plane once per plane).  Destinations are allocated once and touched before timing,
so no variant pays for first-touch page faults -- except the two "fresh" variants, which allocate as a caller does: the
per-plane loop with a zero-filled buffer per plane (the Rust shim's vec![0f32; n]), the bulk call into one np.empty.  Variants are interleaved rep by rep; each figure is the median of
--reps timed runs after three warm-up runs.  Also: the pinned D2H rate by transfer size (what the staging size rests on).
Prints one JSON document."""
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

PLANES = A.PLANES


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def figure(ms_list, nbytes):
    ms = statistics.median(ms_list)
    return {"ms": round(ms, 4), "gb_s": round(nbytes / ms / 1e6, 2), "ms_min": round(min(ms_list), 4),
            "ms_max": round(max(ms_list), 4), "runs": len(ms_list)}


def case(ctx, w, h, keep, reps):
    import torch
    L = A.lib()
    res = ctx.extract_features(A.synth_frame(w, h, 0), keep_all_planes=keep)
    nl = res.counts(0)[0]
    total = res.pyramid_floats()
    nbytes = total * 4
    # per-plane loop: one touched pageable buffer per plane, reused
    planes = []
    for lvl in range(nl):
        for p in range(10):
            n = C.c_uint64()
            A._check(L.akz_fetch_plane(res._h, 0, lvl, p, None, C.byref(n)))
            if n.value:
                planes.append((lvl, p, np.ones(n.value, np.float32)))

    def per_plane():
        n = C.c_uint64()
        for lvl, p, buf in planes:
            A._check(L.akz_fetch_plane(res._h, 0, lvl, p, buf.ctypes.data_as(C.c_void_p), C.byref(n)))

    pageable = np.ones(total, np.float32)
    pinned = torch.ones(total, dtype=torch.float32, pin_memory=True).numpy()

    def ptrs_into(buf):
        ptrs, off = (C.c_void_p * (nl * 10))(), 0
        for lvl in range(nl):
            info = res.level_info(lvl)
            for p in range(10):
                if lvl == 0 and PLANES[p] in ("Lflow", "Lstep"):
                    continue
                ptrs[lvl * 10 + p] = buf.ctypes.data + off * 4
                off += info["w"] * info["h"]
        assert off == total
        return ptrs

    p_pageable, p_pinned = ptrs_into(pageable), ptrs_into(pinned)
    got = C.c_uint64()

    def pyramid(ptrs):
        A._check(L.akz_fetch_pyramid(res._h, 0, ptrs, nl * 10, C.byref(got)))

    dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dev.fill_(1)
    torch.cuda.synchronize()

    def ceiling(buf):
        A._check(L.akz_memcpy_d2h(ctx._h, C.c_void_p(buf.ctypes.data), C.c_void_p(dev.data_ptr()), nbytes))

    def per_plane_fresh():  # the Rust shim's loop: a zero-filled fresh buffer per plane (vec![0f32; n]), then the fetch
        n = C.c_uint64()
        for lvl, p, buf in planes:
            fresh = np.zeros(buf.size, np.float32)
            A._check(L.akz_fetch_plane(res._h, 0, lvl, p, fresh.ctypes.data_as(C.c_void_p), C.byref(n)))

    def pyramid_fresh():  # ExtractResult.pyramid() without `out`: one fresh np.empty
        fresh = np.empty(total, np.float32)
        pyramid(ptrs_into(fresh))

    variants = {
        "per_plane_fresh": per_plane_fresh,
        "pyramid_fresh": pyramid_fresh,
        "per_plane_pageable": per_plane,
        "pyramid_pageable": lambda: pyramid(p_pageable),
        "pyramid_pinned": lambda: pyramid(p_pinned),
        "ceiling_pinned": lambda: ceiling(pinned),
        "ceiling_pageable": lambda: ceiling(pageable),
    }
    times = {k: [] for k in variants}
    for rep in range(3 + reps):
        for k, fn in variants.items():
            ms = timed(fn)
            if rep >= 3:
                times[k].append(ms)
    # the three destinations hold the same bytes, and the bulk call moved all of them
    pyramid(p_pageable)
    pyramid(p_pinned)
    assert got.value == nbytes, (got.value, nbytes)
    per_plane()
    flat = np.concatenate([buf for _, _, buf in planes])
    assert flat.tobytes() == pageable.tobytes() == pinned.tobytes(), "pyramid differs from the per-plane fetch"
    out = {"w": w, "h": h, "planes": "all" if keep else "lean", "levels": nl, "plane_calls": len(planes),
           "bytes": nbytes}
    out.update({k: figure(v, nbytes) for k, v in times.items()})
    cp = out["ceiling_pinned"]["ms"]
    out["pinned_vs_ceiling"] = round(cp / out["pyramid_pinned"]["ms"], 3)
    out["pageable_vs_ceiling"] = round(cp / out["pyramid_pageable"]["ms"], 3)
    out["pageable_speedup_vs_per_plane"] = round(out["per_plane_pageable"]["ms"] / out["pyramid_pageable"]["ms"], 2)
    out["fresh_speedup_vs_per_plane"] = round(out["per_plane_fresh"]["ms"] / out["pyramid_fresh"]["ms"], 2)
    res.close()
    return out


def d2h_by_size(ctx, reps):
    import torch
    L = A.lib()
    out = []
    for mib in (1, 2, 4, 8, 16, 32):
        n = mib << 20
        dev = torch.ones(n, dtype=torch.uint8, device="cuda")
        pin = torch.empty(n, dtype=torch.uint8, pin_memory=True).numpy()
        torch.cuda.synchronize()
        ms = []
        for rep in range(3 + reps):
            t = timed(lambda: A._check(L.akz_memcpy_d2h(ctx._h, C.c_void_p(pin.ctypes.data), C.c_void_p(dev.data_ptr()), n)))
            if rep >= 3:
                ms.append(t)
        out.append({"mib": mib, **figure(ms, n)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5
    import torch
    assert torch.cuda.is_available(), "pyramid_fetch measures on a GPU"
    ctx = A.Context(0, torch.cuda.current_stream().cuda_stream)
    doc = {"tool": "tools/pyramid_fetch.py", "device": torch.cuda.get_device_name(0),
           "host_threads": len(os.sched_getaffinity(0)),
           "cases": [case(ctx, w, h, keep, args.reps) for w, h in ((1920, 1080), (3840, 2160)) for keep in (True, False)],
           "pinned_d2h_by_size": d2h_by_size(ctx, args.reps)}
    ctx.close()
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
