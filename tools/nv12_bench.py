#!/usr/bin/env python
"""Device-resident timing of the NV12 entry points beside their I420 siblings, which move the same bytes with the same arithmetic.

Batches of 1080p frames resident in HBM (seeded noise, BT.709 limited, centre siting, tight layouts).  Cases, each with its I420
leg, its NV12 leg and the library's stream-copy probe (nus_probe_device kind 1) moving the same number of bytes:
  to_rgba_nearest / to_rgba_bilinear   nus_yuv420_to_rgba8_device / nus_nv12_to_rgba8_device
  to_yuv                               nus_rgba8_to_yuv420_device / nus_rgba8_to_nv12_device
  resize                               nus_yuv420_resize_device / nus_nv12_resize_device, 1080p -> 4K, Lanczos-3, FMA mode
  repack                               nus_yuv420_to_nv12_device / nus_nv12_to_yuv420_device (no I420 sibling: the two directions)
hipEvents on the launch stream; every leg warmed, then the legs of a case alternate bracket by bracket in one process
(tools/yuv_bench.py's scheme); each figure is the median of its brackets with the smallest and the largest beside it.  One JSON
line per case: microseconds per frame of each leg, NV12 / I420 with whether the NV12 leg's fastest bracket is slower than the I420
leg's slowest (slower beyond the spread), and copy / leg -- the leg's rate as a fraction of the copy's.  No threshold.
usage: python tools/nv12_bench.py [--size 1920x1080] [--frames 31] [--scale 2] [--reps R] [--rounds 7] [--quick]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the package: torch's HIP runtime first)

import nu_scaler_amd as nsc  # noqa: E402
from nu_scaler_amd import yuv  # noqa: E402
from yuv_bench import timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", type=int, default=31)
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=7, help="timed brackets per leg; the median is reported")
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    ap.add_argument("--quick", action="store_true", help="one warm-up call and one bracket of 1 call per leg")
    args = ap.parse_args()
    if nsc.device_count() < 1:
        raise SystemExit("nv12_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm_seconds = 1, 1, 0.0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    lib = nsc._capi.lib()
    w, h = (int(x) for x in args.size.split("x"))
    ow, oh, n = w * args.scale, h * args.scale, args.frames
    yb, fb, yb_out = yuv.frame_bytes(w, h), w * h * 4, yuv.frame_bytes(ow, oh)
    assert yuv.nv12_frame_bytes(w, h) == yb
    gen = torch.Generator(device=dev).manual_seed(1234 + w)
    d_rgba = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device=dev, generator=gen)
    d_rgba_out = torch.empty_like(d_rgba)
    d_i420, d_nv12 = torch.empty((n, yb), dtype=torch.uint8, device=dev), torch.empty((n, yb), dtype=torch.uint8, device=dev)
    d_i420_out, d_nv12_out = torch.empty_like(d_i420), torch.empty_like(d_nv12)
    d_big = torch.empty((2, n, yb_out), dtype=torch.uint8, device=dev)
    src_fmt = yuv.YuvFormat("bt709", "limited", "center", "bilinear")
    yuv.to_yuv_device(d_rgba.data_ptr(), w, h, d_i420.data_ptr(), src_fmt, n, stream=s)  # real frames, the same in both layouts
    yuv.i420_to_nv12_device(d_i420.data_ptr(), w, h, d_nv12.data_ptr(), n, stream=s)
    planes = yuv.YuvResizer(w, h, ow, oh, "lanczos3", "center", "fma")
    torch.cuda.synchronize()

    def report(case, legs, names, moved, **extra):
        """legs: callables; the last one is the copy probe moving `moved` bytes a frame."""
        brackets = timed_alternating(legs, args.reps, args.warm_seconds, args.rounds)
        us = [[x * 1e3 / n for x in g] for g in brackets]
        med = [g[len(g) // 2] for g in us]
        row = {"case": f"{w}x{h}x{n}_{case}", "frames": n, "brackets": len(us[0]), "calls_per_bracket": args.reps, "bytes_moved_per_frame": moved}
        for name, g, m in zip(names, us, med):
            row.update({f"{name}_us_per_frame": round(m, 2), f"{name}_min": round(g[0], 2), f"{name}_max": round(g[-1], 2),
                        f"{name}_spread_over_median": round((g[-1] - g[0]) / m, 3)})
        for name, m in zip(names[:-1], med[:-1]):
            row[f"{name}_fraction_of_copy_rate"] = round(med[-1] / m, 3)
        row[f"{names[1]}_over_{names[0]}"] = round(med[1] / med[0], 3)
        row[f"{names[1]}_slower_than_{names[0]}_beyond_spread"] = bool(us[1][0] > us[0][-1])
        row.update(extra)
        print(json.dumps(row), flush=True)

    def copier(nbytes):
        nbytes = (n * nbytes // 2) & ~15  # half read, half written: the bytes a leg moves over the bus

        def copy():
            if lib.nus_probe_device(1, d_big[0].data_ptr(), d_big[1].data_ptr(), nbytes, 0, s) != nsc._capi.OK:
                raise RuntimeError(nsc._capi.last_error())

        return copy

    for name, chroma in (("to_rgba_nearest", "nearest"), ("to_rgba_bilinear", "bilinear")):
        fmt = yuv.YuvFormat("bt709", "limited", "center", chroma)
        report(name, [lambda: yuv.to_rgba_device(d_i420.data_ptr(), w, h, d_rgba_out.data_ptr(), fmt, n, stream=s),
                      lambda: yuv.nv12_to_rgba_device(d_nv12.data_ptr(), w, h, d_rgba_out.data_ptr(), fmt, n, stream=s), copier(yb + fb)],
               ("i420", "nv12", "copy"), yb + fb)
    report("to_yuv", [lambda: yuv.to_yuv_device(d_rgba.data_ptr(), w, h, d_i420_out.data_ptr(), src_fmt, n, stream=s),
                      lambda: yuv.rgba_to_nv12_device(d_rgba.data_ptr(), w, h, d_nv12_out.data_ptr(), src_fmt, n, stream=s), copier(yb + fb)],
           ("i420", "nv12", "copy"), yb + fb)
    report(f"resize_to_{ow}x{oh}_lanczos3_fma", [lambda: planes.resize_device(d_i420.data_ptr(), d_big[0].data_ptr(), n, stream=s),
                                                  lambda: planes.resize_nv12_device(d_nv12.data_ptr(), d_big[1].data_ptr(), n, stream=s), copier(yb + yb_out)],
           ("i420", "nv12", "copy"), yb + yb_out)
    report("repack", [lambda: yuv.i420_to_nv12_device(d_i420.data_ptr(), w, h, d_nv12_out.data_ptr(), n, stream=s),
                      lambda: yuv.nv12_to_i420_device(d_nv12.data_ptr(), w, h, d_i420_out.data_ptr(), n, stream=s), copier(2 * yb)],
           ("to_nv12", "to_i420", "copy"), 2 * yb)


if __name__ == "__main__":
    main()
