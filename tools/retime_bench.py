#!/usr/bin/env python
"""Device-resident timing of the frame-rate conversion by a rational ratio (the nus_*_retime_* entry points) against the route a
caller had to take before they existed: one multi-time call per pair with that pair's times plus a hipMemcpyDtoDAsync per real
frame, the schedule walked on the host.  A stream of 121 frames of 1080p (1 GB of frames, every frame the one before moved by a few
pixels, as tools/flow_warps_bench.py), the ratios 5/2, 12/5 and 2/5, five legs:
  dense   flows given: nus_interp_retime_device  |  per pair nus_interp_interpolate_multi_device (FMA warp on both sides);
  flow    estimator + warp, FAST mode: nus_flow_retime_device_stream  |  nus_flow_estimate_device_stream, then the dense per-pair
          route in FMA mode;
  bm      block matching, Medium preset: nus_bm_retime_device_stream  |  nus_bm_estimate_device over all pairs, then per pair
          nus_bm_warp_device (EXACT on both sides);
  select  both flows given, the select warp: nus_interp_retime_select_device  |  per pair nus_interp_interpolate_select_device with that
          pair's times (FMA on both sides);
  select_flow   estimator both ways + select warp, FAST mode: nus_flow_retime_select_device_stream  |
          nus_flow_estimate_both_device_stream, then the select per-pair route in FMA mode.
Both routes of a leg write the same bytes into the same buffer (checked once per case before the timing).  hipEvents on the launch
stream, both routes warmed, then they alternate bracket by bracket in one process; each figure is the median of its brackets with
the smallest and the largest beside it, in microseconds per OUTPUT frame.  One JSON line per case.
usage: python tools/retime_bench.py [--legs dense,flow,bm,select,select_flow] [--ratios 5/2,12/5,2/5] [--frames 121] [--reps R] [--rounds N] [--quick]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the package: torch's HIP runtime first)

import nu_scaler_amd as nsc  # noqa: E402
from nu_scaler_amd import synthetic as syn  # noqa: E402
from nu_scaler_amd.retime import retime_schedule  # noqa: E402


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


def pair_plan(n_frames, num, den):
    """The schedule as the per-pair route walks it: [(pair, first in-between output, its times)] and [(output, real frame)]."""
    pairs, reals, sched = [], [], retime_schedule(n_frames, den, num)
    for j, e in enumerate(sched):
        if e.rem == 0:
            reals.append((j, e.pair))
        elif pairs and pairs[-1][0] == e.pair:
            pairs[-1][2].append(e.t)
        else:
            pairs.append((e.pair, j, [e.t]))
    return pairs, reals, len(sched)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="dense,flow,bm,select,select_flow")
    ap.add_argument("--ratios", default="5/2,12/5,2/5")
    ap.add_argument("--frames", type=int, default=121)
    ap.add_argument("--reps", type=int, default=2, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=7, help="timed brackets per route; the median is reported")
    ap.add_argument("--warm-seconds", type=float, default=0.5)
    ap.add_argument("--quick", action="store_true", help="one warm-up call and one bracket of 1 call per route")
    args = ap.parse_args()
    if nsc.device_count() < 1:
        raise SystemExit("retime_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm_seconds = 1, 1, 0.0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    w, h, n_frames = 1920, 1080, args.frames
    n, fb = n_frames - 1, 1920 * 1080 * 4
    frames = syn.noise_stream_torch(n_frames, w, h, dev)
    for k in range(n):
        frames[k + 1] = torch.roll(frames[k], (5 - 2 * (k % 6), 3 * (k % 7) - 9), (0, 1))
    base = frames.data_ptr()
    flows = torch.empty((n, h, w, 2), dtype=torch.float32, device=dev)
    fe = nsc.FlowEstimator(levels=3, coarse_iterations=50, refine_iterations=10)
    fe.set_mode("fast")
    fe.estimate_device_stream(base, n_frames, w, h, flows.data_ptr(), s)  # the dense leg's given flows
    flows_bwd = None
    if "select" in args.legs:  # the select legs' second flow: every pair B -> A
        flows_bwd = torch.empty((n, h, w, 2), dtype=torch.float32, device=dev)
        fe.estimate_both_device_stream(base, n_frames, w, h, flows.data_ptr(), flows_bwd.data_ptr(), s)
    d_bwd = flows_bwd.data_ptr() if flows_bwd is not None else 0
    it = nsc.WgpuFrameInterpolator()
    it.set_mode("fma")
    bm = nsc.BlockMatcher("medium")
    bx, by = bm.block_grid(w, h)
    vectors = torch.empty((n, by, bx, 2), dtype=torch.int16, device=dev)
    bm_ws_bytes = max(bm.stream_workspace_size(w, h, n_frames), bm.workspace_size(w, h, n))
    bm_ws = torch.empty(bm_ws_bytes + 16, dtype=torch.uint8, device=dev)
    d_bm_ws = (bm_ws.data_ptr() + 15) & ~15
    torch.cuda.synchronize()

    for ratio in args.ratios.split(","):
        num, den = (int(x) for x in ratio.split("/"))
        pairs, reals, n_out = pair_plan(n_frames, num, den)
        out = torch.empty((n_out, fb), dtype=torch.uint8, device=dev)
        d_out = out.data_ptr()

        def copy_reals():
            for j, k in reals:
                out[j].copy_(frames[k].view(-1), non_blocking=True)  # hipMemcpyDtoDAsync on the launch stream

        def dense_pairs():
            for k, j, ts in pairs:
                it.interpolate_multi_device(base + k * fb, fb, base + (k + 1) * fb, fb, flows.data_ptr() + k * w * h * 8, w, h, ts,
                                            d_out + j * fb, 0, 1, s)
            copy_reals()

        def flow_pairs():
            fe.estimate_device_stream(base, n_frames, w, h, flows.data_ptr(), s)
            dense_pairs()

        def select_pairs():
            for k, j, ts in pairs:
                it.interpolate_select_device(base + k * fb, fb, base + (k + 1) * fb, fb, flows.data_ptr() + k * w * h * 8, d_bwd + k * w * h * 8,
                                             w, h, ts, d_out + j * fb, 0, 1, s)
            copy_reals()

        def select_flow_pairs():
            fe.estimate_both_device_stream(base, n_frames, w, h, flows.data_ptr(), d_bwd, s)
            select_pairs()

        def bm_pairs():
            bm.estimate_device(base, fb, base + fb, fb, w, h, n, d_bm_ws, bm_ws_bytes, vectors.data_ptr(), stream=s)
            for k, j, ts in pairs:
                bm.warp_device(base + k * fb, fb, base + (k + 1) * fb, fb, w, h, 1, vectors[k].data_ptr(), d_out + j * fb, times=ts,
                               mode="exact", stream=s)
            copy_reals()

        legs = {
            "dense": ("nus_interp_retime_device", lambda: it.retime_device(base, fb, n_frames, flows.data_ptr(), w, h, num, den, d_out, 0, s),
                      dense_pairs),
            "flow": ("nus_flow_retime_device_stream",
                     lambda: fe.retime_device_stream(base, n_frames, w, h, num, den, d_out, flows.data_ptr(), 0, s), flow_pairs),
            "bm": ("nus_bm_retime_device_stream",
                   lambda: bm.retime_stream_device(base, fb, n_frames, w, h, num, den, d_bm_ws, bm_ws_bytes, d_out, mode="exact",
                                                   d_vectors=vectors.data_ptr(), stream=s), bm_pairs),
            "select": ("nus_interp_retime_select_device",
                       lambda: it.retime_select_device(base, fb, n_frames, flows.data_ptr(), d_bwd, w, h, num, den, d_out, 0, s), select_pairs),
            "select_flow": ("nus_flow_retime_select_device_stream",
                            lambda: fe.retime_select_device_stream(base, n_frames, w, h, num, den, d_out, flows.data_ptr(), d_bwd, 0, s),
                            select_flow_pairs),
        }
        for leg in args.legs.split(","):
            entry, one_launch, per_pair = legs[leg]
            out.fill_(0x5A)
            one_launch()
            first = out.clone()
            out.fill_(0xA5)
            per_pair()
            same = bool(torch.equal(first, out))
            del first
            brackets = timed_alternating([one_launch, per_pair], args.reps, args.warm_seconds, args.rounds)
            us = [[x * 1e3 / n_out for x in g] for g in brackets]
            med = [g[len(g) // 2] for g in us]
            print(json.dumps({"case": f"{w}x{h}x{n_frames}_{leg}_{num}_{den}", "leg": leg, "entry": entry, "ratio": ratio, "frames_in": n_frames,
                              "frames_out": n_out, "pairs_with_outputs": len(pairs), "real_frames": len(reals), "same_bytes": same,
                              "brackets": len(us[0]), "calls_per_bracket": args.reps,
                              "one_launch_us_per_output": round(med[0], 2), "one_launch_min": round(us[0][0], 2),
                              "one_launch_max": round(us[0][-1], 2), "per_pair_us_per_output": round(med[1], 2),
                              "per_pair_min": round(us[1][0], 2), "per_pair_max": round(us[1][-1], 2),
                              "one_launch_over_per_pair": round(med[0] / med[1], 3)}), flush=True)
        del out
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
