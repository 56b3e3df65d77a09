#!/usr/bin/env python
"""Device-resident timing of the flow estimator's re-linearisation mode (nus_flow_set_warps): nus_flow_estimate_device_stream on a
stream of 32 frames of 1080p (31 pairs; 265 MB of frames, every frame the one before moved by a few pixels, as the stream of
tools/blockmatch_bench.py --stream), 3 levels, 50 + 10 steps, for warps = 0, 1, 2 in EXACT and in FAST mode.  hipEvents on the
launch stream, every leg warmed, then the legs of a mode alternate bracket by bracket in one process; each figure is the median of
its brackets, and the smallest and largest bracket are printed beside it.  warps = 0 on the same binary in the same call is the
baseline of the ratios.  One JSON line per case.
--median: the median mode instead (nus_flow_set_median): for EXACT and FAST at warps 1 and 2 the legs median 0 / 3 / 5 alternate the
same way, and median 0 at the same warps is the baseline of the ratios.
--project: the warp's projection rounds instead (nus_flow_set_project / nus_interp_set_flow_project): rounds 0 / 1 / 2 / 3 of
nus_flow_interpolate_device_stream (EXACT and FAST estimator, t = 0.5) and of nus_interp_interpolate_multi_device (3 times per pair,
EXACT and FMA warp, on the flows of one estimate), the legs alternating the same way, rounds 0 the baseline of the ratios.
--project-rounds 0 times the baseline alone and touches none of the new settings, so the same file also runs on a build from
before the setting existed.
--bidirectional: the select warp and the estimator's bidirectional setting instead (nus_interp_interpolate_select_device,
nus_flow_set_bidirectional): per projection round count of --project-rounds (default here 0,3) and K = 1 and K = 3 times per pair,
the plain warp (nus_interp_interpolate_multi_device: k_warp_blend_flow, or k_warp_blend_flow_proj with rounds) against the select
warp on the same forward flows plus the backward ones, EXACT and FMA; then nus_flow_interpolate_device_stream with the setting off
against on, EXACT and FAST estimator, at the last round count.  Off and on alternate in one process; off is the baseline.
usage: python tools/flow_warps_bench.py [--median | --project [--project-rounds 0,1,2,3] | --bidirectional [--project-rounds 0,3]]
                                        [--reps R] [--rounds N] [--frames F] [--quick]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the package: torch's HIP runtime first)

import nu_scaler_amd as nsc  # noqa: E402
from nu_scaler_amd import synthetic as syn  # noqa: E402

WARPS = (0, 1, 2)
MEDIAN_WARPS = (1, 2)  # --median: the settings the mode is meant for
MEDIANS = (0, 3, 5)
PROJECT_TIMES = [0.25, 0.5, 0.75]  # --project: the multi-time warp's time set


def timed_alternating(fns, reps, warm_seconds, rounds):
    """Every leg warmed, then `rounds` times one bracket of each in turn -> per leg the sorted ms per call of its brackets."""
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


def project_legs(args, frames, flows, w, h, n_frames, s):
    n = n_frames - 1
    fb = w * h * 4
    rounds = [int(r) for r in args.project_rounds.split(",")]
    if not rounds or rounds[0] != 0:
        raise SystemExit("flow_warps_bench: --project-rounds starts with 0, the baseline")
    mid = torch.empty((n, len(PROJECT_TIMES), h, w, 4), dtype=torch.uint8, device=frames.device)

    def report(case, extra, brackets):
        us = [[x * 1e3 / n for x in g] for g in brackets]
        med = [g[len(g) // 2] for g in us]
        for r, g, m in zip(rounds, us, med):
            print(json.dumps(dict({"case": f"{w}x{h}x{n}_{case}_project{r}", "width": w, "height": h, "pairs": n, "project": r}, **extra,
                                  **{"working_set_bytes": frames.numel(), "brackets": len(g), "calls_per_bracket": args.reps,
                                     "us_per_pair": round(m, 2), "us_per_pair_min": round(g[0], 2), "us_per_pair_max": round(g[-1], 2),
                                     "over_project0": round(m / med[0], 3)})), flush=True)

    for mode in ("exact", "fast"):  # estimator + warp through one entry point
        handles = []
        for r in rounds:
            fe = nsc.FlowEstimator(levels=3, coarse_iterations=50, refine_iterations=10)
            fe.set_mode(mode)
            if r:
                fe.set_project(r)
            handles.append(fe)
        legs = [lambda fe=fe: fe.interpolate_device_stream(frames.data_ptr(), n_frames, w, h, 0.5, mid.data_ptr(), flows.data_ptr(), s)
                for fe in handles]
        report(f"interpolate_device_stream_{mode}", {"entry": "nus_flow_interpolate_device_stream", "mode": mode, "levels": 3,
                                                     "coarse_iterations": 50, "refine_iterations": 10},
               timed_alternating(legs, args.reps, args.warm_seconds, args.rounds))
        del handles, legs
        torch.cuda.synchronize()
    for mode in ("exact", "fma"):  # the warp alone, on the flows the last estimate left
        handles = []
        for r in rounds:
            it = nsc.WgpuFrameInterpolator()
            it.set_mode(mode)
            if r:
                it.set_flow_project(r)
            handles.append(it)
        legs = [lambda it=it: it.interpolate_multi_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, flows.data_ptr(), w, h,
                                                          PROJECT_TIMES, mid.data_ptr(), 0, n, s) for it in handles]
        report(f"interpolate_multi_device_{mode}", {"entry": "nus_interp_interpolate_multi_device", "mode": mode,
                                                    "times": len(PROJECT_TIMES)},
               timed_alternating(legs, args.reps, args.warm_seconds, args.rounds))
        del handles, legs
        torch.cuda.synchronize()


def bidirectional_legs(args, frames, flows, w, h, n_frames, s):
    n = n_frames - 1
    fb = w * h * 4
    rounds = [int(r) for r in args.project_rounds.split(",")]
    mid = torch.empty((n, len(PROJECT_TIMES), h, w, 4), dtype=torch.uint8, device=frames.device)
    bwd = torch.empty_like(flows)
    fe = nsc.FlowEstimator(levels=3, coarse_iterations=50, refine_iterations=10)
    fe.estimate_device_stream(frames.data_ptr(), n_frames, w, h, flows.data_ptr(), s)
    for k in range(n):  # the flows B -> A of the same pairs
        fe.estimate_device(frames[k + 1].data_ptr(), frames[k].data_ptr(), w, h, bwd[k].data_ptr(), s)
    torch.cuda.synchronize()
    del fe

    def report(case, extra, brackets):
        us = [[x * 1e3 / n for x in g] for g in brackets]
        med = [g[len(g) // 2] for g in us]
        for on, g, m in zip((0, 1), us, med):
            print(json.dumps(dict({"case": f"{w}x{h}x{n}_{case}_bidirectional{on}", "width": w, "height": h, "pairs": n, "bidirectional": on},
                                  **extra, **{"working_set_bytes": frames.numel(), "brackets": len(g), "calls_per_bracket": args.reps,
                                              "us_per_pair": round(m, 2), "us_per_pair_min": round(g[0], 2),
                                              "us_per_pair_max": round(g[-1], 2), "over_off": round(m / med[0], 3)})), flush=True)

    for mode in ("exact", "fma"):  # the warp alone
        for r in rounds:
            for times in (PROJECT_TIMES[1:2], PROJECT_TIMES):
                it = nsc.WgpuFrameInterpolator()
                it.set_mode(mode)
                it.set_flow_project(r)
                legs = [lambda: it.interpolate_multi_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, flows.data_ptr(), w, h, times,
                                                            mid.data_ptr(), 0, n, s),
                        lambda: it.interpolate_select_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, flows.data_ptr(),
                                                             bwd.data_ptr(), w, h, times, mid.data_ptr(), 0, n, s)]
                report(f"warp_{mode}_project{r}_times{len(times)}", {"entry": "nus_interp_interpolate_multi_device / _select_device",
                                                                      "mode": mode, "project": r, "times": len(times)},
                       timed_alternating(legs, args.reps, args.warm_seconds, args.rounds))
                torch.cuda.synchronize()
    for mode in ("exact", "fast"):  # estimator + warp through one entry point
        handles = []
        for on in (False, True):
            fe = nsc.FlowEstimator(levels=3, coarse_iterations=50, refine_iterations=10, project=rounds[-1], bidirectional=on)
            fe.set_mode(mode)
            handles.append(fe)
        legs = [lambda fe=fe: fe.interpolate_device_stream(frames.data_ptr(), n_frames, w, h, 0.5, mid.data_ptr(), flows.data_ptr(), s)
                for fe in handles]
        report(f"interpolate_device_stream_{mode}_project{rounds[-1]}", {"entry": "nus_flow_interpolate_device_stream", "mode": mode,
                                                                          "project": rounds[-1], "levels": 3, "coarse_iterations": 50,
                                                                          "refine_iterations": 10},
               timed_alternating(legs, args.reps, args.warm_seconds, args.rounds))
        del handles, legs
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=7, help="timed brackets per leg; the median is reported")
    ap.add_argument("--warm-seconds", type=float, default=0.5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--quick", action="store_true", help="one warm-up call and one bracket of 2 calls per leg")
    ap.add_argument("--median", action="store_true", help="time median 0 / 3 / 5 at warps 1 and 2 instead of warps 0 / 1 / 2")
    ap.add_argument("--project", action="store_true", help="time the warp's projection rounds instead (see the module text)")
    ap.add_argument("--project-rounds", default=None, help="with --project: the legs (comma-separated round counts, 0 first; default "
                                                           "0,1,2,3); with --bidirectional: the round counts timed (default 0,3)")
    ap.add_argument("--bidirectional", action="store_true", help="time the select warp and the bidirectional estimator against the "
                                                                 "forward-only route instead (see the module text)")
    args = ap.parse_args()
    if args.median + args.project + args.bidirectional > 1:
        ap.error("--median, --project and --bidirectional exclude each other")
    if args.project_rounds is None:
        args.project_rounds = "0,3" if args.bidirectional else "0,1,2,3"
    if nsc.device_count() < 1:
        raise SystemExit("flow_warps_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm_seconds = 2, 1, 0.0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    w, h, n_frames = 1920, 1080, args.frames
    n = n_frames - 1
    frames = syn.noise_stream_torch(n_frames, w, h, dev)
    for k in range(n):
        frames[k + 1] = torch.roll(frames[k], (5 - 2 * (k % 6), 3 * (k % 7) - 9), (0, 1))
    flows = torch.empty((n, h, w, 2), dtype=torch.float32, device=dev)
    if args.project:
        return project_legs(args, frames, flows, w, h, n_frames, s)
    if args.bidirectional:
        return bidirectional_legs(args, frames, flows, w, h, n_frames, s)
    for mode, warps in [(m, wn) for m in ("exact", "fast") for wn in MEDIAN_WARPS] if args.median else []:
        handles = []
        for median in MEDIANS:
            fe = nsc.FlowEstimator(levels=3, coarse_iterations=50, refine_iterations=10, warps=warps, median=median)
            fe.set_mode(mode)
            handles.append(fe)
        legs = [lambda fe=fe: fe.estimate_device_stream(frames.data_ptr(), n_frames, w, h, flows.data_ptr(), s) for fe in handles]
        brackets = timed_alternating(legs, args.reps, args.warm_seconds, args.rounds)
        us = [[x * 1e3 / n for x in g] for g in brackets]
        med = [g[len(g) // 2] for g in us]
        for median, g, m in zip(MEDIANS, us, med):
            print(json.dumps({"case": f"{w}x{h}x{n}_{mode}_warps{warps}_median{median}", "width": w, "height": h, "pairs": n, "mode": mode,
                              "warps": warps, "median": median, "levels": 3, "coarse_iterations": 50, "refine_iterations": 10,
                              "working_set_bytes": frames.numel(), "brackets": len(g), "calls_per_bracket": args.reps,
                              "us_per_pair": round(m, 2), "us_per_pair_min": round(g[0], 2), "us_per_pair_max": round(g[-1], 2),
                              "over_median0": round(m / med[0], 3)}), flush=True)
        del handles, legs
        torch.cuda.synchronize()
    for mode in () if args.median else ("exact", "fast"):
        handles = []
        for warps in WARPS:
            fe = nsc.FlowEstimator(levels=3, coarse_iterations=50, refine_iterations=10, warps=warps)
            fe.set_mode(mode)
            handles.append(fe)
        legs = [lambda fe=fe: fe.estimate_device_stream(frames.data_ptr(), n_frames, w, h, flows.data_ptr(), s) for fe in handles]
        brackets = timed_alternating(legs, args.reps, args.warm_seconds, args.rounds)
        us = [[x * 1e3 / n for x in g] for g in brackets]
        med = [g[len(g) // 2] for g in us]
        for warps, g, m in zip(WARPS, us, med):
            print(json.dumps({"case": f"{w}x{h}x{n}_{mode}_warps{warps}", "width": w, "height": h, "pairs": n, "mode": mode, "warps": warps,
                              "levels": 3, "coarse_iterations": 50, "refine_iterations": 10, "working_set_bytes": frames.numel(),
                              "brackets": len(g), "calls_per_bracket": args.reps, "us_per_pair": round(m, 2),
                              "us_per_pair_min": round(g[0], 2), "us_per_pair_max": round(g[-1], 2),
                              "over_warps0": round(m / med[0], 3)}), flush=True)
        del handles, legs
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
