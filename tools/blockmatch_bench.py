#!/usr/bin/env python
"""Device-resident timing of the block-matching motion estimator (nus_bm_estimate_device): hipEvents on the launch stream,
warm-up, then the median of several timed brackets.  One JSON line per case:
  pairs of 1080p (32) and 4K (8), the three presets (High 8 / 24, Medium 16 / 16, Low 32 / 8), on shifted noise.
Every pair has frames of its own: 2n distinct frames per case, 531 MB at both sizes, twice the 256 MiB Infinity Cache.
Per case, us per pair of
  estimate             search + confidence pass, vectors / SADs / flags out;
  estimate_flow        the same plus the dense flow as 2 x f16 per pixel;
  estimate_flow_warp   the same plus the dense-flow warp (nus_interp_interpolate_device, FMA mode, t = 0.5) reading that flow;
the floor of the search -- candidates x pixels byte-SAD lane-operations at 78.6 T lane-operations/s (157.3 TFLOPS FP32 vector
/ 2 per FMA), an estimate from shapes -- and the fraction of it reached.  A last line times the FAST Horn-Schunck flow stream
(nus_flow_estimate_device_stream, tools/flow_stream_bench.py's mode 9) on 33 frames of 1080p in the same process: the project's
other estimator.
usage: python tools/blockmatch_bench.py [--reps R] [--rounds N] [--quick]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the package: torch's HIP runtime first)

import nu_scaler_amd as nsc  # noqa: E402
from nu_scaler_amd import synthetic as syn  # noqa: E402

VALU_LANE_OPS_PER_S = 157.3e12 / 2
PRESETS = (("high", 8, 24), ("medium", 16, 16), ("low", 32, 8))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=5, help="timed brackets per case; the median is reported")
    ap.add_argument("--warm-seconds", type=float, default=0.5)
    ap.add_argument("--quick", action="store_true", help="one warm-up call and one bracket of 2 calls per case (profiling runs)")
    args = ap.parse_args()
    if nsc.device_count() < 1:
        raise SystemExit("blockmatch_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm_seconds = 2, 1, 0.0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    it = nsc.WgpuFrameInterpolator()
    it.set_flow_format("f16")
    it.set_mode("fma")
    for w, h, n in ((1920, 1080, 32), (3840, 2160, 8)):
        fb = w * h * 4
        # 2n frames back to back; pair i = (frame i, frame n + i), B = A moved by (3 i - 9, 5 - 2 i) pixels
        frames = syn.noise_stream_torch(2 * n, w, h, dev)
        for i in range(n):
            frames[n + i] = torch.roll(frames[i], (5 - 2 * i, 3 * i - 9), (0, 1))
        base, base_b = frames.data_ptr(), frames.data_ptr() + n * fb
        flow = torch.empty((n, h, w, 2), dtype=torch.float16, device=dev)
        mid = torch.empty((n, h, w, 4), dtype=torch.uint8, device=dev)
        for name, bs, radius in PRESETS:
            bm = nsc.BlockMatcher(name)
            nbx, nby = bm.block_grid(w, h)
            ws_n = bm.workspace_size(w, h, n)
            ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
            vec = torch.empty((n, nby, nbx, 2), dtype=torch.int16, device=dev)
            sad = torch.empty((n, nby, nbx), dtype=torch.int32, device=dev)
            flags = torch.empty((n, nby, nbx), dtype=torch.uint8, device=dev)

            def estimate(d_flow=0):
                bm.estimate_device(base, fb, base_b, fb, w, h, n, ws.data_ptr(), ws_n, vec.data_ptr(), sad.data_ptr(), flags.data_ptr(),
                                   d_flow, "f16", s)

            def whole():
                estimate(flow.data_ptr())
                it.interpolate_device(base, fb, base_b, fb, flow.data_ptr(), w, h, 0.5, mid.data_ptr(), n, s)

            us = [timed(f, args.reps, args.warm_seconds, args.rounds) * 1e3 / n
                  for f in (estimate, lambda: estimate(flow.data_ptr()), whole)]
            floor_us = (2 * radius + 1) ** 2 * w * h / VALU_LANE_OPS_PER_S * 1e6
            print(json.dumps({"case": f"{w}x{h}x{n}_{name}", "width": w, "height": h, "pairs": n, "block_size": bs, "search_radius": radius,
                              "working_set_bytes": frames.numel(), "us_per_pair_estimate": round(us[0], 2),
                              "us_per_pair_estimate_flow": round(us[1], 2), "us_per_pair_estimate_flow_warp": round(us[2], 2),
                              "search_floor_us_per_pair": round(floor_us, 2), "fraction_of_search_floor": round(floor_us / us[0], 3),
                              "flow_expansion_share_of_whole": round((us[1] - us[0]) / us[2], 3),
                              "warp_share_of_whole": round((us[2] - us[1]) / us[2], 3)}), flush=True)
            del ws, vec, sad, flags
        del frames, flow, mid
        torch.cuda.synchronize()
    w, h, n = 1920, 1080, 33
    frames = syn.gradient_stream_torch(n, w, h, dev) // 2 + syn.noise_stream_torch(n, w, h, dev) // 2
    flows = torch.empty((n - 1, h, w, 2), dtype=torch.float32, device=dev)
    fe = nsc.FlowEstimator(levels=3, coarse_iterations=50, refine_iterations=10)
    fe.set_mode("fast")
    fe.set_tiled(1)
    ms = timed(lambda: fe.estimate_device_stream(frames.data_ptr(), n, w, h, flows.data_ptr(), s), args.reps, args.warm_seconds,
               args.rounds)
    print(json.dumps({"case": f"{w}x{h}x{n - 1}_horn_schunck_fast_stream", "width": w, "height": h, "pairs": n - 1,
                      "us_per_pair_estimate": round(ms * 1e3 / (n - 1), 2)}), flush=True)


if __name__ == "__main__":
    main()
