#!/usr/bin/env python
"""Device-resident timing of the YUV 4:2:0 conversions (nus_yuv420_to_rgba8_device, nus_rgba8_to_yuv420_device) against the
library's own stream-copy probe (nus_probe_device kind 1) moving the same number of bytes in the same process.

Batches of 1080p and 2160p frames resident in HBM (seeded noise, BT.709 limited, centre siting); the cases are both directions,
and towards RGBA the nearest and the bilinear chroma filter.  A conversion moves 5.5 bytes per pixel (1.5 of YUV, 4 of RGBA); the
copy is given (yuv + rgba bytes) / 2 bytes to read and as many to write, so both move the same bytes over the memory bus.
hipEvents on the launch stream, both warmed, then they alternate bracket by bracket (tools/retime_bench.py's scheme); each figure
is the median of its brackets with the smallest and the largest beside it.  One JSON line per case: microseconds per frame of the
conversion and of the copy, and copy / conversion -- the conversion's rate as a fraction of the copy's.  No threshold.
usage: python tools/yuv_bench.py [--sizes 1920x1080,3840x2160] [--frames N] [--reps R] [--rounds N] [--quick]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the package: torch's HIP runtime first)

import nu_scaler_amd as nsc  # noqa: E402
from nu_scaler_amd import yuv  # noqa: E402


def timed_alternating(fns, reps, warm_seconds, rounds):
    """Every route warmed, then `rounds` times one bracket of each in turn -> per route the sorted ms per call of its brackets."""
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < warm_seconds:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
    got = [[] for _ in fns]
    for _ in range(max(1, rounds)):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            got[i].append(a.elapsed_time(b) / reps)
    return [sorted(g) for g in got]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--frames", type=int, default=0, help="frames per batch (0: 64 of 1080p, 16 of 2160p -- about 0.7 GB a batch)")
    ap.add_argument("--reps", type=int, default=4, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=7, help="timed brackets per route; the median is reported")
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    ap.add_argument("--quick", action="store_true", help="one warm-up call and one bracket of 1 call per route")
    args = ap.parse_args()
    if nsc.device_count() < 1:
        raise SystemExit("yuv_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm_seconds = 1, 1, 0.0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    lib = nsc._capi.lib()
    for size in args.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        n = args.frames or max(1, 64 * 1920 * 1080 // (w * h))
        yb, fb = yuv.frame_bytes(w, h), w * h * 4
        gen = torch.Generator(device=dev).manual_seed(1234 + w)
        d_yuv = torch.randint(0, 256, (n, yb), dtype=torch.uint8, device=dev, generator=gen)
        d_rgba = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device=dev, generator=gen)
        d_yuv_out, d_rgba_out = torch.empty_like(d_yuv), torch.empty_like(d_rgba)
        copy_bytes = (n * (yb + fb) // 2) & ~15
        src, dst = d_rgba.data_ptr(), d_rgba_out.data_ptr()  # (the largest buffers: the copy fits in them)
        cases = [("to_rgba_nearest", "nearest", True), ("to_rgba_bilinear", "bilinear", True), ("to_yuv", "bilinear", False)]
        for name, chroma, to_rgba in cases:
            fmt = yuv.YuvFormat("bt709", "limited", "center", chroma)
            if to_rgba:
                conv = lambda: yuv.to_rgba_device(d_yuv.data_ptr(), w, h, d_rgba_out.data_ptr(), fmt, n, stream=s)  # noqa: E731
            else:
                conv = lambda: yuv.to_yuv_device(d_rgba.data_ptr(), w, h, d_yuv_out.data_ptr(), fmt, n, stream=s)  # noqa: E731

            def copy():
                if lib.nus_probe_device(1, src, dst, copy_bytes, 0, s) != nsc._capi.OK:
                    raise RuntimeError(nsc._capi.last_error())

            brackets = timed_alternating([conv, copy], args.reps, args.warm_seconds, args.rounds)
            us = [[x * 1e3 / n for x in g] for g in brackets]
            med = [g[len(g) // 2] for g in us]
            moved = n * (yb + fb)
            print(json.dumps({"case": f"{w}x{h}x{n}_{name}", "direction": "to_rgba" if to_rgba else "to_yuv", "chroma_filter": chroma if to_rgba else None,
                              "siting": "center", "frames": n, "bytes_moved_per_frame": yb + fb, "brackets": len(us[0]),
                              "calls_per_bracket": args.reps, "convert_us_per_frame": round(med[0], 2), "convert_min": round(us[0][0], 2),
                              "convert_max": round(us[0][-1], 2), "copy_us_per_frame": round(med[1], 2), "copy_min": round(us[1][0], 2),
                              "copy_max": round(us[1][-1], 2), "convert_gb_per_s": round(moved / n / med[0] / 1e3, 1),
                              "copy_gb_per_s": round(2 * copy_bytes / n / med[1] / 1e3, 1),
                              "fraction_of_copy_rate": round(med[1] / med[0], 3)}), flush=True)
        del d_yuv, d_rgba, d_yuv_out, d_rgba_out
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
