#!/usr/bin/env python
"""Device-resident timing of the image-quality metrics (nus_metrics_compare_device): hipEvents on the launch stream, warm-up,
then the median of several timed brackets (tools/quick_bench.py's `timed`).  One JSON line per case:
  pairs of 1080p (32) and 4K (8), MSE only / SSIM only / both, gradient and noise content (nu_scaler_amd/synthetic.py).
Every pair has frames of its own: 2n distinct frames per case, 531 MB at both sizes, twice the 256 MiB Infinity Cache, so a call
and the next one back to back read their frames from HBM, not from a cache a shared or replayed frame would sit in.
Each line gives us per pair, the GB/s of frame bytes read (2 frames per pair), and the fraction of the bound that applies:
  MSE only  -> HBM: 2 * W * H * 4 bytes per pair over 8 TB/s;
  SSIM      -> VALU: an estimate of 130 lane-operations per channel and valid centre (5 statistics x 11 taps x 2 passes, the
               products and the ratio), 3 channels, at 78.6 T lane-operations/s (157.3 TFLOPS FP32 vector / 2 per FMA).
usage: python tools/metrics_bench.py [--reps R] [--rounds N] [--quick]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the package: torch's HIP runtime first)

import nu_scaler_amd as nsc  # noqa: E402
from nu_scaler_amd import metrics  # noqa: E402
from nu_scaler_amd import synthetic as syn  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
VALU_LANE_OPS_PER_S = 157.3e12 / 2
OPS_PER_CHANNEL_CENTRE = 130


def timed(fn, reps, warm_seconds=1.0, rounds=5):
    import time

    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_seconds:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    got = []
    for _ in range(max(1, rounds)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        got.append(a.elapsed_time(b) / reps)
    got.sort()
    return got[len(got) // 2]


def floors(w, h, what):
    """(seconds at the HBM bound, seconds at the VALU bound) of one pair."""
    hbm = 2 * w * h * 4 / HBM_BYTES_PER_S
    valu = 3 * (w - 10) * (h - 10) * OPS_PER_CHANNEL_CENTRE / VALU_LANE_OPS_PER_S if what != "mse" else 0.0
    return hbm, valu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=5, help="timed brackets per case; the median is reported")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--quick", action="store_true", help="one warm-up call and one bracket of 2 calls per case (profiling runs)")
    args = ap.parse_args()
    if nsc.device_count() < 1:
        raise SystemExit("metrics_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm_seconds = 2, 1, 0.0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for w, h, n in ((1920, 1080, 32), (3840, 2160, 8)):
        fb = w * h * 4
        for pattern in ("gradient", "noise"):
            # 2n frames back to back; pair i = (frame i, frame n + i): no frame is read twice in a call
            frames = (syn.gradient_stream_torch(2 * n, w, h, dev) if pattern == "gradient" else syn.noise_stream_torch(2 * n, w, h, dev))
            base, base_b = frames.data_ptr(), frames.data_ptr() + n * fb
            working_set = frames.numel()
            for what in ("mse", "ssim", "both"):
                mse, ssim = what != "ssim", what != "mse"
                ws_n = metrics.workspace_size(w, h, n, mse=mse, ssim=ssim)
                ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
                out = torch.empty(3 * n, dtype=torch.float64, device=dev)

                def run():
                    metrics.compare_device(base, fb, base_b, fb, w, h, n, ws.data_ptr(), ws_n, out.data_ptr(), mse=mse, ssim=ssim,
                                           stream=s)

                ms = timed(run, args.reps, args.warm_seconds, args.rounds)
                us_pair = ms * 1e3 / n
                hbm, valu = floors(w, h, what)
                bound = "hbm" if hbm >= valu else "valu"
                floor = max(hbm, valu)
                print(json.dumps({"case": f"{w}x{h}x{n}_{pattern}_{what}", "width": w, "height": h, "pairs": n, "pattern": pattern,
                                  "metrics": what, "working_set_bytes": working_set, "us_per_pair": round(us_pair, 3),
                                  "gb_per_s_read": round(2 * fb / (us_pair * 1e-6) / 1e9, 1), "bound": bound,
                                  "floor_us_per_pair": round(floor * 1e6, 2), "fraction_of_bound": round(floor / (us_pair * 1e-6), 3)}),
                      flush=True)
                del ws, out
            del frames
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
