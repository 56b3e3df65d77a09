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
--stream: instead, frame generation over a device-resident stream of 65 frames of 1080p (64 distinct pairs, 539 MB), per preset and
per K in {1, 3, 7} in-between frames per pair, FMA mode, us per pair of
  stream        nus_bm_interpolate_multi_device_stream: search, confidence pass, the warp straight from the block vectors;
  dense_route   the same frames from the entry points that were there before: nus_bm_estimate_device with an F16 flow, then
                nus_interp_interpolate_multi_device reading it;
  bm_warp       nus_bm_warp_device alone, on the vectors of the stream;
  dense_warp    nus_interp_interpolate_multi_device alone, on their expanded flow;
  flow_expand   k_bm_flow's share: nus_bm_estimate_device with the flow minus without.
--bidirectional: instead, the forward-backward check (nus_bm_set_bidirectional) on and off, per preset, on 32 pairs of 1080p (the
working set of the estimator's case; content that moves, so that the searches agree on most blocks), us per pair of
  estimate_off / estimate_on   nus_bm_estimate_device with vectors, SADs and flags out, two handles of one binary;
  stream_off / stream_on       nus_bm_interpolate_multi_device_stream over the same 33 frames, K = 1, FMA mode;
and the ratios on / off: the mode's cost is the second search.
The legs of a case alternate in one process, bracket by bracket; each figure is the median of its brackets.
usage: python tools/blockmatch_bench.py [--reps R] [--rounds N] [--quick] [--stream | --bidirectional]"""
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


def timed_alternating(fns, reps, warm_seconds=0.5, rounds=5):
    """The legs of one case side by side: every leg warmed, then `rounds` times one bracket of each in turn -> median ms per call."""
    import time

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
    return [sorted(g)[len(g) // 2] for g in got]


def stream_legs(args):
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    w, h, n_frames = 1920, 1080, 65
    n, fb = n_frames - 1, 1920 * 1080 * 4
    # every frame the one before moved by a few pixels: 64 distinct pairs
    frames = syn.noise_stream_torch(n_frames, w, h, dev)
    for k in range(n):
        frames[k + 1] = torch.roll(frames[k], (5 - 2 * (k % 6), 3 * (k % 7) - 9), (0, 1))
    base = frames.data_ptr()
    flow = torch.empty((n, h, w, 2), dtype=torch.float16, device=dev)
    it = nsc.WgpuFrameInterpolator()
    it.set_flow_format("f16")
    it.set_mode("fma")
    for K in (1, 3, 7):
        times = [0.5] if K == 1 else nsc.frame_times(K + 1)
        mid = torch.empty((n, K, h, w, 4), dtype=torch.uint8, device=dev)
        mid_d = torch.empty((n, K, h, w, 4), dtype=torch.uint8, device=dev)
        for name, bs, radius in PRESETS:
            bm = nsc.BlockMatcher(name)
            nbx, nby = bm.block_grid(w, h)
            ws_n, sws_n = bm.workspace_size(w, h, n), bm.stream_workspace_size(w, h, n_frames)
            ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
            sws = torch.empty(sws_n, dtype=torch.uint8, device=dev)
            vec = torch.empty((n, nby, nbx, 2), dtype=torch.int16, device=dev)

            def estimate(d_flow=0):
                bm.estimate_device(base, fb, base + fb, fb, w, h, n, ws.data_ptr(), ws_n, vec.data_ptr(), 0, 0, d_flow, "f16", s)

            def dense_warp():
                it.interpolate_multi_device(base, fb, base + fb, fb, flow.data_ptr(), w, h, times, mid_d.data_ptr(), 0, n, s)

            def dense_route():
                estimate(flow.data_ptr())
                dense_warp()

            def stream():
                bm.interpolate_stream_device(base, fb, n_frames, w, h, sws.data_ptr(), sws_n, mid.data_ptr(), times=times, mode="fma",
                                             stream=s)

            def bm_warp():
                bm.warp_device(base, fb, base + fb, fb, w, h, n, vec.data_ptr(), mid.data_ptr(), times=times, mode="fma", stream=s)

            dense_route()  # vec and flow hold this preset's motion for the warp-alone legs
            stream()
            torch.cuda.synchronize()
            same = bool(torch.equal(mid, mid_d))
            legs = [stream, dense_route, bm_warp, dense_warp, estimate, lambda: estimate(flow.data_ptr())]
            ms = timed_alternating(legs, args.reps, args.warm_seconds, args.rounds)
            us = [round(x * 1e3 / n, 2) for x in ms]
            row = {"case": f"{w}x{h}x{n}_{name}_K{K}_stream", "width": w, "height": h, "pairs": n, "block_size": bs,
                   "search_radius": radius, "n_times": K, "mode": "fma", "working_set_bytes": frames.numel(),
                   "stream_equals_dense_route_bytes": same, "us_per_pair_stream": us[0], "us_per_pair_dense_route": us[1],
                   "stream_over_dense_route": round(us[0] / us[1], 3), "us_per_pair_bm_warp": us[2], "us_per_pair_dense_warp": us[3],
                   "us_per_pair_flow_expand": round(us[5] - us[4], 2),
                   "bm_warp_over_dense_warp_plus_expand": round(us[2] / (us[3] + us[5] - us[4]), 3)}
            print(json.dumps(row), flush=True)
            del ws, sws, vec
        del mid, mid_d
        torch.cuda.synchronize()


def bidirectional_legs(args):
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    w, h, n_frames = 1920, 1080, 33
    n, fb = n_frames - 1, 1920 * 1080 * 4
    frames = syn.noise_stream_torch(n_frames, w, h, dev)
    for k in range(n):
        frames[k + 1] = torch.roll(frames[k], (5 - 2 * (k % 6), 3 * (k % 7) - 9), (0, 1))
    base = frames.data_ptr()
    mid = torch.empty((n, 1, h, w, 4), dtype=torch.uint8, device=dev)
    for name, bs, radius in PRESETS:
        legs, keep, flagged = [], [], 0
        for on in (False, True):
            bm = nsc.BlockMatcher(name, bidirectional=on)
            nbx, nby = bm.block_grid(w, h)
            ws_n, sws_n = bm.workspace_size(w, h, n), bm.stream_workspace_size(w, h, n_frames)
            ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
            sws = torch.empty(sws_n, dtype=torch.uint8, device=dev)
            vec = torch.empty((n, nby, nbx, 2), dtype=torch.int16, device=dev)
            sad = torch.empty((n, nby, nbx), dtype=torch.int32, device=dev)
            flags = torch.empty((n, nby, nbx), dtype=torch.uint8, device=dev)

            def estimate(bm=bm, ws=ws, ws_n=ws_n, vec=vec, sad=sad, flags=flags):
                bm.estimate_device(base, fb, base + fb, fb, w, h, n, ws.data_ptr(), ws_n, vec.data_ptr(), sad.data_ptr(), flags.data_ptr(),
                                   0, "f16", s)

            def stream(bm=bm, sws=sws, sws_n=sws_n):
                bm.interpolate_stream_device(base, fb, n_frames, w, h, sws.data_ptr(), sws_n, mid.data_ptr(), times=[0.5], mode="fma",
                                             stream=s)

            legs += [estimate, stream]
            keep.append((bm, ws, sws, vec, sad, flags))
            if on:
                estimate()
                torch.cuda.synchronize()
                flagged = int((flags != 0).sum())
        legs = [legs[0], legs[2], legs[1], legs[3]]  # estimate off, on, stream off, on
        ms = timed_alternating(legs, args.reps, args.warm_seconds, args.rounds)
        us = [round(x * 1e3 / n, 2) for x in ms]
        print(json.dumps({"case": f"{w}x{h}x{n}_{name}_bidirectional", "width": w, "height": h, "pairs": n, "block_size": bs,
                          "search_radius": radius, "working_set_bytes": frames.numel(), "blocks_repaired": flagged,
                          "blocks": n * keep[1][3].shape[1] * keep[1][3].shape[2], "us_per_pair_estimate_off": us[0],
                          "us_per_pair_estimate_on": us[1], "estimate_on_over_off": round(us[1] / us[0], 3),
                          "us_per_pair_stream_off": us[2], "us_per_pair_stream_on": us[3],
                          "stream_on_over_off": round(us[3] / us[2], 3)}), flush=True)
        del keep, legs
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=5, help="timed brackets per case; the median is reported")
    ap.add_argument("--warm-seconds", type=float, default=0.5)
    ap.add_argument("--quick", action="store_true", help="one warm-up call and one bracket of 2 calls per case (profiling runs)")
    ap.add_argument("--stream", action="store_true", help="the stream legs (see above) instead of the estimator's cases")
    ap.add_argument("--bidirectional", action="store_true", help="the forward-backward check on and off (see above) instead")
    args = ap.parse_args()
    if nsc.device_count() < 1:
        raise SystemExit("blockmatch_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm_seconds = 2, 1, 0.0
    if args.stream:
        return stream_legs(args)
    if args.bidirectional:
        return bidirectional_legs(args)
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
