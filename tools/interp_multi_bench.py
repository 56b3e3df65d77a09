#!/usr/bin/env python
"""Several in-between frames per pair from one launch against K single-time launches of the same pairs (dev tool).  One JSON
line per case:
  1080p and 4K; zero flow, dense flow F32 in EXACT and in FMA mode, F16 in FMA mode; K = 1, 2, 3, 7 (times k / (K + 1));
  the motion stream (1080p, FAST estimator, K = 3): nus_flow_interpolate_multi_device_stream against K single-time stream calls.
Each case runs in one process, the multi-time launch and the K single-time launches alternated bracket by bracket; hipEvent
timing after warm-up, the median bracket reported.  The pairs are distinct (A and B of their own) and span at least 512 MB, so
their frames come from HBM, not from the 256 MiB Infinity Cache.  Algorithmic bytes per pair = A + B + flow + K frames out
(the single-time launches move A + B + flow once per time).
usage: python tools/interp_multi_bench.py [--reps R] [--rounds N] [--quick] [--no-motion]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the package: torch's HIP runtime first)

import nu_scaler_amd as nsc  # noqa: E402
from nu_scaler_amd.interpolator import frame_times  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
MIN_WORKING_SET = 512 << 20


def bracket(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, rounds, warm):
    """Median ms per call of each function, brackets alternated."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    got = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            got[i].append(bracket(fn, reps))
    return [sorted(g)[len(g) // 2] for g in got]


def line(**kw):
    print(json.dumps(kw), flush=True)


def warp_cases(args, s):
    dev = torch.device("cuda:0")
    it = nsc.WgpuFrameInterpolator()
    for w, h in ((1920, 1080), (3840, 2160)):
        fb = w * h * 4
        n = -(-MIN_WORKING_SET // (2 * fb))  # pairs: 2n distinct frames of at least 512 MB
        A = torch.randint(0, 256, (n, h, w, 4), dtype=torch.uint8, device=dev)
        B = torch.randint(0, 256, (n, h, w, 4), dtype=torch.uint8, device=dev)
        g = torch.Generator(device=dev).manual_seed(3)
        coarse = torch.randn((n, 2, h // 40, w // 40), generator=g, device=dev) * 4.0
        f32 = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear").permute(0, 2, 3, 1).contiguous()
        f16 = f32.to(torch.float16)
        del coarse
        out = torch.empty(n * max(args.ks) * fb, dtype=torch.uint8, device=dev)
        for case, flow, mode, ffmt in (("zero", None, "exact", "f32"), ("dense_f32_exact", f32, "exact", "f32"),
                                       ("dense_f32_fma", f32, "fma", "f32"), ("dense_f16_fma", f16, "fma", "f16")):
            it.set_mode(mode)
            it.set_flow_format(ffmt)
            fl = flow.data_ptr() if flow is not None else 0
            flow_bytes = 0 if flow is None else w * h * (8 if ffmt == "f32" else 4)
            for K in args.ks:
                times = frame_times(K + 1)

                def multi():
                    it.interpolate_multi_device(A.data_ptr(), fb, B.data_ptr(), fb, fl, w, h, times, out.data_ptr(), 0, n, s)

                def singles():
                    for k, t in enumerate(times):
                        it.interpolate_device(A.data_ptr(), fb, B.data_ptr(), fb, fl, w, h, t, out.data_ptr() + k * n * fb, n, s)

                ms_multi, ms_single = alternate([multi, singles], args.reps, args.rounds, args.warm)
                us_m, us_s = ms_multi * 1e3 / n, ms_single * 1e3 / n
                bytes_pair = 2 * fb + flow_bytes + K * fb
                line(case=case, width=w, height=h, K=K, pairs=n, working_set_bytes=2 * n * fb + n * flow_bytes,
                     us_per_pair_multi=round(us_m, 3), us_per_pair_singles=round(us_s, 3), multi_over_singles=round(us_m / us_s, 3),
                     bytes_per_pair=bytes_pair, tb_per_s_multi=round(bytes_pair / (us_m * 1e-6) / 1e12, 3),
                     fraction_of_8tbps_multi=round(bytes_pair / (us_m * 1e-6) / HBM_BYTES_PER_S, 3),
                     fraction_of_8tbps_singles=round(K * (2 * fb + flow_bytes + fb) / (us_s * 1e-6) / HBM_BYTES_PER_S, 3))
        del A, B, f32, f16, out
        torch.cuda.synchronize()


def motion_cases(args, s):
    from nu_scaler_amd import synthetic as syn

    dev = torch.device("cuda:0")
    w, h, n_frames, K = 1920, 1080, 17, 3
    fb, n = w * h * 4, n_frames - 1
    frames = syn.gradient_stream_torch(n_frames, w, h, dev)
    mid = torch.empty(n * K * fb, dtype=torch.uint8, device=dev)
    times = frame_times(K + 1)
    fe = nsc.FlowEstimator()
    fe.set_mode("fast")
    for ffmt in ("f16", "f32"):
        def multi():
            fe.interpolate_multi_device_stream(frames.data_ptr(), n_frames, w, h, times, mid.data_ptr(), 0, 0, s, flow_format=ffmt)

        def singles():
            for k, t in enumerate(times):
                fe.interpolate_device_stream(frames.data_ptr(), n_frames, w, h, t, mid.data_ptr() + k * n * fb, 0, s, flow_format=ffmt)

        ms_multi, ms_single = alternate([multi, singles], max(1, args.reps // 2), args.rounds, args.warm)
        us_m, us_s = ms_multi * 1e3 / n, ms_single * 1e3 / n
        line(case=f"motion_fast_{ffmt}", width=w, height=h, K=K, pairs=n, us_per_pair_multi=round(us_m, 3),
             us_per_pair_singles=round(us_s, 3), multi_over_singles=round(us_m / us_s, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=5, help="brackets per side; the median is reported")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls per side")
    ap.add_argument("--ks", default="1,2,3,7")
    ap.add_argument("--quick", action="store_true", help="one bracket of 2 calls per side (profiling runs)")
    ap.add_argument("--no-motion", action="store_true")
    args = ap.parse_args()
    args.ks = [int(k) for k in args.ks.split(",")]
    if nsc.device_count() < 1:
        raise SystemExit("interp_multi_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm = 2, 1, 1
    s = torch.cuda.current_stream().cuda_stream
    warp_cases(args, s)
    if not args.no_motion:
        motion_cases(args, s)


if __name__ == "__main__":
    main()
