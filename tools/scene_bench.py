#!/usr/bin/env python
"""Device-resident timing of the scene-cut detector (nus_scene_detect_device, nus_scene_apply_cuts_device): hipEvents on the
launch stream, warm-up, then the median of several timed brackets (as tools/metrics_bench.py).  One JSON line per case:
  pairs of 1080p (32) and 4K (8), gradient and noise content; detect alone; apply behind a 4x time set with 0 % and 100 % of the
  pairs cut; and the box's own yardsticks, the figures of bench.py's `roofline.copy_ceiling` taken with the same probes
  (nus_probe_device) over the same frames in the same process: a read-only stream (kind 3: the detector reads and writes next
  to nothing, so this is the ceiling of its access pattern), the 16-B-per-lane stream copy (kind 1, read + written bytes) and
  hipMemcpyDtoDAsync (kind 0); and a one-workgroup launch (the floor under an apply pass that finds no cut).
Every pair has frames of its own: 2n distinct frames per case, 531 MB at both sizes, twice the 256 MiB Infinity Cache, so a call
and the next one back to back read their frames from HBM.  --build NAME labels the lines (A/B runs of a library built with a
dev macro, loaded through NUS_LIB_PATH).
usage: python tools/scene_bench.py [--reps R] [--rounds N] [--quick] [--build NAME]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the package: torch's HIP runtime first)

import nu_scaler_amd as nsc  # noqa: E402
from nu_scaler_amd import _capi as C  # noqa: E402
from nu_scaler_amd import synthetic as syn  # noqa: E402
from nu_scaler_amd.interpolator import frame_times  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=10, help="calls per timed bracket")
    ap.add_argument("--rounds", type=int, default=5, help="timed brackets per case; the median is reported")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--quick", action="store_true", help="one warm-up call and one bracket of 2 calls per case (profiling runs)")
    ap.add_argument("--build", default="default", help="label of the library build, copied into every detect line")
    args = ap.parse_args()
    if nsc.device_count() < 1:
        raise SystemExit("scene_bench: no HIP device")
    if args.quick:
        args.reps, args.rounds, args.warm_seconds = 2, 1, 0.0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    lib = C.lib()
    det = nsc.SceneDetector()
    times = frame_times(4)
    tiny = torch.zeros(64, dtype=torch.uint8, device=dev)
    launch_ms = timed(lambda: lib.nus_probe_device(3, tiny.data_ptr(), tiny.data_ptr() + 32, 16, 0, s), args.reps, args.warm_seconds,
                      args.rounds)
    print(json.dumps({"case": "one_workgroup_launch", "us_per_call": round(launch_ms * 1e3, 3)}), flush=True)
    for w, h, n in ((1920, 1080, 32), (3840, 2160, 8)):
        fb = w * h * 4
        for pattern in ("gradient", "noise"):
            # 2n frames back to back; pair i = (frame i, frame n + i): no frame is read twice in a call
            frames = (syn.gradient_stream_torch(2 * n, w, h, dev) if pattern == "gradient" else syn.noise_stream_torch(2 * n, w, h, dev))
            base, base_b = frames.data_ptr(), frames.data_ptr() + n * fb
            ws_n = det.workspace_size(w, h, n)
            ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
            meas = torch.empty(16 * n, dtype=torch.uint8, device=dev)
            cut = torch.empty(n, dtype=torch.uint8, device=dev)
            common = {"width": w, "height": h, "pairs": n, "pattern": pattern, "working_set_bytes": frames.numel()}

            ms = timed(lambda: det.detect_device(base, fb, base_b, fb, w, h, n, ws.data_ptr(), ws_n, cut.data_ptr(), meas.data_ptr(),
                                                 stream=s), args.reps, args.warm_seconds, args.rounds)
            read_ms = timed(lambda: lib.nus_probe_device(3, base, tiny.data_ptr(), 2 * n * fb, 0, s), args.reps, args.warm_seconds,
                            args.rounds)
            # copies of the first n frames onto the last n: n * fb bytes read and as many written
            copy_ms = timed(lambda: lib.nus_probe_device(1, base, base_b, n * fb, 0, s), args.reps, args.warm_seconds, args.rounds)
            dtod_ms = timed(lambda: lib.nus_probe_device(0, base, base_b, n * fb, 0, s), args.reps, args.warm_seconds, args.rounds)
            frames.copy_(syn.gradient_stream_torch(2 * n, w, h, dev) if pattern == "gradient" else syn.noise_stream_torch(2 * n, w, h, dev))
            gbs, copy_gbs, dtod_gbs = 2 * n * fb / (ms * 1e-3) / 1e9, 2 * n * fb / (copy_ms * 1e-3) / 1e9, 2 * n * fb / (dtod_ms * 1e-3) / 1e9
            print(json.dumps(dict(common, case=f"{w}x{h}x{n}_{pattern}_detect", build=args.build, us_per_pair=round(ms * 1e3 / n, 3),
                                  gb_per_s_read=round(gbs, 1),
                                  read_only_stream_gb_per_s=round(2 * n * fb / (read_ms * 1e-3) / 1e9, 1),
                                  fraction_of_read_only_stream=round(read_ms / ms, 3),
                                  stream_copy_float4_gb_per_s=round(copy_gbs, 1), fraction_of_stream_copy=round(gbs / copy_gbs, 3),
                                  hipMemcpyDtoDAsync_gb_per_s=round(dtod_gbs, 1), fraction_of_hipMemcpyDtoD=round(gbs / dtod_gbs, 3))),
                  flush=True)
            out = torch.empty(n * len(times) * fb, dtype=torch.uint8, device=dev)
            for percent in (0, 100):
                cut.fill_(1 if percent else 0)
                ms = timed(lambda: det.apply_cuts_device(base, fb, base_b, fb, w, h, times, cut.data_ptr(), out.data_ptr(), 0, n, stream=s),
                           args.reps, args.warm_seconds, args.rounds)
                moved = (2 + len(times)) * n * fb if percent else 0  # A and B read once, every frame of the time set written
                print(json.dumps(dict(common, case=f"{w}x{h}x{n}_{pattern}_apply_{percent}pct_cut", n_times=len(times),
                                      us_per_call=round(ms * 1e3, 3), us_per_pair=round(ms * 1e3 / n, 3),
                                      gb_per_s_moved=round(moved / (ms * 1e-3) / 1e9, 1),
                                      one_workgroup_launch_us=round(launch_ms * 1e3, 3))), flush=True)
            del frames, ws, meas, cut, out
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
