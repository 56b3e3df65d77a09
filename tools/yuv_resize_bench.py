#!/usr/bin/env python
"""Device-resident timing of the two routes from RGBA frames to up-scaled I420 frames, and of the plane resize alone.

From the same batch of RGBA frames resident in HBM (seeded noise, BT.709 limited, centre siting; default 31 frames of 1080p to 4K,
Lanczos-3 in FMA mode):
  (a) rgb route     upscale_device at the target size, then to_yuv_device at the target size   (video's scale_domain="rgb")
  (b) planar route  to_yuv_device at the source size, then YuvResizer.resize_device            (scale_domain="yuv")
  (c) plane resize  YuvResizer.resize_device alone
  copy              the library's stream-copy probe (nus_probe_device kind 1) moving the bytes (c) moves: the source and the
                    target I420 frame, 15.55 MB a frame at 1080p -> 4K, half of them read and half written
hipEvents on the launch stream around synchronised work; every route warmed, then they alternate bracket by bracket in one process
(tools/yuv_bench.py's scheme); each figure is the median of its brackets with the smallest and the largest beside it.  One JSON
line per case: microseconds per frame, (b) / (a) with the brackets' spread, and copy / (c) -- the plane resize's rate as a fraction
of the copy's.  No threshold.
usage: python tools/yuv_resize_bench.py [--size 1920x1080] [--scale 2] [--frames 31] [--algorithm lanczos3] [--siting center]
                                        [--reps R] [--rounds 7] [--quick]"""
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
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--frames", type=int, default=31)
    ap.add_argument("--algorithm", default="lanczos3")
    ap.add_argument("--siting", default="center")
    ap.add_argument("--reps", type=int, default=2, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=7, help="timed brackets per route; the median is reported")
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    ap.add_argument("--quick", action="store_true", help="one warm-up call and one bracket of 1 call per route")
    args = ap.parse_args()
    if nsc.device_count() < 1:
        raise SystemExit("yuv_resize_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm_seconds = 1, 1, 0.0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    lib = nsc._capi.lib()
    w, h = (int(x) for x in args.size.split("x"))
    ow, oh, n = w * args.scale, h * args.scale, args.frames
    yb_in, yb_out, fb_in, fb_out = yuv.frame_bytes(w, h), yuv.frame_bytes(ow, oh), w * h * 4, ow * oh * 4
    gen = torch.Generator(device=dev).manual_seed(1234 + w)
    d_rgba = torch.randint(0, 256, (n, fb_in), dtype=torch.uint8, device=dev, generator=gen)
    d_big = torch.empty((n, fb_out), dtype=torch.uint8, device=dev)
    d_small_yuv = torch.empty((n, yb_in), dtype=torch.uint8, device=dev)
    d_out_a, d_out_b = torch.empty((n, yb_out), dtype=torch.uint8, device=dev), torch.empty((n, yb_out), dtype=torch.uint8, device=dev)
    fmt = yuv.YuvFormat("bt709", "limited", args.siting, "bilinear")
    up = nsc.PyWgpuUpscaler("quality", args.algorithm)
    up.initialize(w, h, ow, oh)
    planes = yuv.YuvResizer(w, h, ow, oh, args.algorithm, args.siting, "fma")
    yuv.to_yuv_device(d_rgba.data_ptr(), w, h, d_small_yuv.data_ptr(), fmt, n, stream=s)  # (c)'s input: real frames, not noise planes
    torch.cuda.synchronize()

    def rgb_route():
        up.upscale_device(d_rgba.data_ptr(), d_big.data_ptr(), n, s)
        yuv.to_yuv_device(d_big.data_ptr(), ow, oh, d_out_a.data_ptr(), fmt, n, stream=s)

    def planar_route():
        yuv.to_yuv_device(d_rgba.data_ptr(), w, h, d_small_yuv.data_ptr(), fmt, n, stream=s)
        planes.resize_device(d_small_yuv.data_ptr(), d_out_b.data_ptr(), n, stream=s)

    def plane_resize():
        planes.resize_device(d_small_yuv.data_ptr(), d_out_b.data_ptr(), n, stream=s)

    copy_bytes = (n * (yb_in + yb_out) // 2) & ~15

    def copy():
        if lib.nus_probe_device(1, d_big.data_ptr(), d_big.data_ptr() + (n * fb_out // 2 & ~15), copy_bytes, 0, s) != nsc._capi.OK:
            raise RuntimeError(nsc._capi.last_error())

    brackets = timed_alternating([rgb_route, planar_route, plane_resize, copy], args.reps, args.warm_seconds, args.rounds)
    us = [[x * 1e3 / n for x in g] for g in brackets]
    med = [g[len(g) // 2] for g in us]
    spread = [round((g[-1] - g[0]) / m, 3) for g, m in zip(us, med)]
    print(json.dumps({"case": f"{w}x{h}->{ow}x{oh}x{n}_{args.algorithm}_fma_{args.siting}", "frames": n, "brackets": len(us[0]),
                      "calls_per_bracket": args.reps,
                      "a_rgb_route_us_per_frame": round(med[0], 2), "a_min": round(us[0][0], 2), "a_max": round(us[0][-1], 2),
                      "b_planar_route_us_per_frame": round(med[1], 2), "b_min": round(us[1][0], 2), "b_max": round(us[1][-1], 2),
                      "c_plane_resize_us_per_frame": round(med[2], 2), "c_min": round(us[2][0], 2), "c_max": round(us[2][-1], 2),
                      "copy_us_per_frame": round(med[3], 2), "copy_min": round(us[3][0], 2), "copy_max": round(us[3][-1], 2),
                      "bracket_spread_over_median": {"a": spread[0], "b": spread[1], "c": spread[2], "copy": spread[3]},
                      "b_over_a": round(med[1] / med[0], 3), "b_faster_than_a_beyond_spread": bool(us[1][-1] < us[0][0]),
                      "c_bytes_moved_per_frame": yb_in + yb_out, "c_gb_per_s": round((yb_in + yb_out) / med[2] / 1e3, 1),
                      "copy_gb_per_s": round(2 * copy_bytes / n / med[3] / 1e3, 1),
                      "c_fraction_of_copy_rate": round(med[3] / med[2], 3)}), flush=True)


if __name__ == "__main__":
    main()
