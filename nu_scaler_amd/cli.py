"""`python -m nu_scaler_amd.cli` -- the image-file commands of the north star's `nu_scaler_cli`
(SURVEY.md section 8f rank 2): `upscale <in.png> <out.png> --algorithm --scale`, following the
legacy crate's `upscale_image_file` (Nu_scale/src/upscale/mod.rs:307-338) and the option names of
its `fullscreen` subcommand (Nu_scale/src/main.rs:36-73: --tech, --quality, --algorithm); `interpolate <a.png> <b.png> <out.png>`
with zero flow, `--flow` (Horn-Schunck) or `--method block_matching [--quality high|medium|low] [--bidirectional]`; `compare <a.png> <b.png>`
prints the `ErrorMetrics` of two images (Nu_scale/src/upscale/common.rs:475-543); `scene <a.png> <b.png>` prints the scene-cut
detector's verdict on the pair, and `interpolate --multiplier M --scene-detect` writes repeats instead of blends across a cut;
`retime --from 24 --to 60 OUT_%04d.png IN0.png IN1.png ...` converts a PNG sequence by a rational frame-rate ratio
(`--flow-bidirectional`: with the select warp, here and in `video`);
`video IN.y4m OUT.y4m (--to FPS | --multiplier M)` does the same for a YUV4MPEG2 file of 4:2:0 frames, window by window, with an
optional `--scale S --algorithm A` up-scale of every output frame (`--scale-domain yuv`: of its Y, U and V planes themselves).
Everything runs on the HIP device; without one the command fails (no CPU path).
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="nu_scaler_cli", description="NU_Scaler image tools on the HIP path")
    sub = ap.add_subparsers(dest="command", required=True)
    up = sub.add_parser("upscale", help="upscale a PNG")
    up.add_argument("input")
    up.add_argument("output")
    up.add_argument("--tech", default="fallback", help="fsr, fallback or none (Nu_scale/src/main.rs:46-52)")
    up.add_argument("--quality", default="quality", help="ultra, quality, balanced or performance")
    up.add_argument("--algorithm", default=None,
                    help="nearest, bilinear, bicubic, lanczos3, triangle, fsr1, easu (default: by quality)")
    up.add_argument("--scale", type=float, default=2.0, help="scale factor (output = trunc(input * scale))")
    up.add_argument("--device", type=int, default=0)
    it = sub.add_parser("interpolate", help="in-between frame of two PNGs of equal size")
    it.add_argument("frame_a")
    it.add_argument("frame_b")
    it.add_argument("output")
    it.add_argument("--t", type=float, default=None, help="time of the new frame between A (0) and B (1); default 0.5")
    it.add_argument("--multiplier", type=int, default=None,
                    help="frame-rate multiplier M (2 .. NUS_INTERP_MAX_TIMES + 1 = 8): the M - 1 frames at t = k / M, written as <stem>_<k><ext>")
    it.add_argument("--flow", action="store_true", help="estimate motion (pyramid + Horn-Schunck) instead of zero flow")
    it.add_argument("--flow-warps", type=int, default=None,
                    help="with --flow: rounds per finer pyramid level that re-linearise about the flow so far (0 .. 4; default 0)")
    it.add_argument("--flow-median", type=int, default=None,
                    help="with --flow: median-filter the flow after every Jacobi run, window 3 or 5 (0, the default: off; meant for "
                         "--flow-warps >= 1)")
    it.add_argument("--flow-project", type=int, default=None,
                    help="with --flow: projection rounds of the warp -- the flow looked up where each output pixel's content came "
                         "from (0 .. 4; default 0)")
    it.add_argument("--flow-bidirectional", action="store_true",
                    help="with --flow: estimate the motion both ways, A -> B and B -> A, and warp each pixel with the vector whose "
                         "two samples agree better (the select warp)")
    it.add_argument("--method", default=None, help="block_matching: the full-search block matcher supplies the motion field")
    it.add_argument("--quality", default="medium", help="block matching preset: high (8 / 24), medium (16 / 16) or low (32 / 8)")
    it.add_argument("--bidirectional", action="store_true",
                    help="with --method block_matching: search both ways and repair the blocks the two searches disagree on")
    it.add_argument("--bidir-tolerance", type=int, default=None,
                    help="with --bidirectional: L1 distance (0 .. 96) within which two vectors answer each other (default 2)")
    it.add_argument("--scene-detect", action="store_true",
                    help="with --multiplier: if the scene-cut detector flags the pair, write repeats of the nearer frame, not blends")
    it.add_argument("--device", type=int, default=0)
    rt = sub.add_parser("retime", help="frame-rate conversion of a PNG sequence by a rational ratio: retime --from 24 --to 60 "
                                       "OUT_%04d.png IN0.png IN1.png ...")
    rt.add_argument("output_pattern", help="where output frame j goes, with one %%d conversion: OUT_%%04d.png")
    rt.add_argument("inputs", nargs="*", help="the input frames in order, at least 2, of one size")
    rt.add_argument("--from", dest="fps_in", required=True, help="input rate: an integer or a fraction such as 24000/1001")
    rt.add_argument("--to", dest="fps_out", required=True, help="output rate, likewise; to/from reduced has terms <= 4096 and is <= 8")
    rt.add_argument("--method", default="optical_flow", help="optical_flow (default), block_matching or blend (zero flow)")
    rt.add_argument("--flow-warps", type=int, default=None, help="optical_flow: re-linearisation rounds per finer level (0 .. 4)")
    rt.add_argument("--flow-median", type=int, default=None, help="optical_flow: median window behind every Jacobi run (0, 3 or 5)")
    rt.add_argument("--flow-project", type=int, default=None, help="optical_flow: projection rounds of the warp (0 .. 4)")
    rt.add_argument("--flow-bidirectional", action="store_true",
                    help="optical_flow: estimate every pair both ways and warp each pixel with the vector whose two samples agree "
                         "better (the select warp)")
    rt.add_argument("--bidirectional", action="store_true", help="block_matching: the forward-backward check")
    rt.add_argument("--scene-detect", action="store_true", help="across a scene cut write repeats of the nearer frame, not blends")
    rt.add_argument("--device", type=int, default=0)
    vd = sub.add_parser("video", help="frame-rate conversion (and up-scaling) of a YUV4MPEG2 file of 8-bit 4:2:0 frames: video IN.y4m "
                                      "OUT.y4m --to 60")
    vd.add_argument("input", help="IN.y4m: C420jpeg, C420mpeg2 or C420, progressive")
    vd.add_argument("output", help="OUT.y4m")
    vd.add_argument("--to", dest="fps_out", default=None, help="output rate: an integer or a fraction such as 60000/1001")
    vd.add_argument("--multiplier", type=int, default=None, help="output rate as a multiple of the input's (1 .. 8) instead of --to")
    vd.add_argument("--method", default="optical_flow", help="optical_flow (default), block_matching or blend (zero flow)")
    vd.add_argument("--scale", type=int, default=1, help="up-scale every output frame by this integer factor (1 .. 4; default 1: off)")
    vd.add_argument("--algorithm", default="lanczos3", help="with --scale: nearest, bilinear, bicubic, lanczos3, triangle")
    vd.add_argument("--scale-domain", dest="scale_domain", choices=("rgb", "yuv"), default="rgb",
                    help="with --scale: rgb (default) up-scales the RGBA frames and converts them to YUV; yuv resamples the Y, U and V "
                         "planes themselves (bicubic, lanczos3 or triangle; even sizes)")
    vd.add_argument("--matrix", default=None, help="bt601 or bt709 (default: bt709 from 720 rows up, else bt601)")
    vd.add_argument("--window", type=int, default=None,
                    help="input frames on the device at a time, at least den + 1 of the reduced ratio (default: from the free memory)")
    vd.add_argument("--scene-detect", action="store_true", help="across a scene cut write repeats of the nearer frame, not blends")
    vd.add_argument("--flow-warps", type=int, default=None, help="optical_flow: re-linearisation rounds per finer level (0 .. 4)")
    vd.add_argument("--flow-median", type=int, default=None, help="optical_flow: median window behind every Jacobi run (0, 3 or 5)")
    vd.add_argument("--flow-project", type=int, default=None, help="optical_flow: projection rounds of the warp (0 .. 4)")
    vd.add_argument("--flow-bidirectional", action="store_true",
                    help="optical_flow: estimate every pair both ways and warp each pixel with the vector whose two samples agree "
                         "better (the select warp)")
    vd.add_argument("--bidirectional", action="store_true", help="block_matching: the forward-backward check")
    vd.add_argument("--device", type=int, default=0)
    sc = sub.add_parser("scene", help="scene-cut detector on two PNGs of equal size: prints cut=0|1 mad=.. hist_permille=..")
    sc.add_argument("a")
    sc.add_argument("b")
    sc.add_argument("--mad", type=int, default=20, help="mean-absolute-difference threshold, 0 .. 255 (a setting, not a measurement)")
    sc.add_argument("--hist", type=int, default=400, help="luma-histogram threshold in permille, 0 .. 1000 (likewise)")
    sc.add_argument("--device", type=int, default=0)
    cp = sub.add_parser("compare", help="MSE, PSNR and SSIM of two PNGs of equal size (ErrorMetrics, "
                                         "Nu_scale/src/upscale/common.rs:475-543)")
    cp.add_argument("a")
    cp.add_argument("b")
    cp.add_argument("--device", type=int, default=0)
    st = sub.add_parser("stream", help="the sharded frame-queue stream: a synthetic 1080p stream through interpolate + x2 upscale "
                                       "on N GPUs of this node, one process per GPU, frames sharded, LUTs broadcast over RCCL")
    st.add_argument("--gpus", type=int, default=1, help="ranks = GPUs of this node (started as a child process tree)")
    st.add_argument("--units", type=int, default=60, help="source frames per GPU (weak scaling: the stream has gpus x units)")
    st.add_argument("--width", type=int, default=1920)
    st.add_argument("--height", type=int, default=1080)
    st.add_argument("--steps", type=int, default=5)
    st.add_argument("--warmup", type=int, default=1)
    st.add_argument("--pattern", default="gradient", choices=["gradient", "noise"])
    st.add_argument("--schedule", default="unit", choices=["unit", "three-stage", "fused"])
    st.add_argument("--algorithm", default="lanczos3", help="an exact-x2 resize filter: lanczos3, bicubic, triangle")
    st.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="nccl = RCCL over xGMI; gloo: rehearsal")
    st.add_argument("--force-device", type=int, default=-1, help="every rank on this device (rehearsal on a one-GPU box)")
    st.add_argument("--no-bind", action="store_true", help="leave the ranks' CPU affinity alone")
    st.add_argument("--digest", action="store_true", help="also print one digest per unit of the stream (sharding-invariant)")
    st.add_argument("--window", type=int, default=0,
                    help="0: every rank holds its whole shard in HBM and repeats it --steps times; W > 0: ONE pass over the stream in "
                         "windows of W units per rank, the next window fetched beside the current one (a stream that need not fit)")
    st.add_argument("--host-fed-seconds", type=float, default=0.0,
                    help="afterwards, every rank feeds its GPU from HOST memory through upscale_batch for this long (mode ii)")
    return ap


def _stream_in_windows(args, S) -> dict:
    """`stream --window W`: one pass over the stream, every rank's shard in windows (ShardedStream.run_windows)."""
    s = S.ShardedStream(args.units * args.gpus, args.width, args.height, source=S.SyntheticSource(args.pattern), backend=args.backend,
                        bind=not args.no_bind, force_device=args.force_device, schedule=args.schedule, algorithm=args.algorithm,
                        resident=False)
    try:
        digests = []

        def consume(st, first, n, mid, up_real, up_mid):
            if args.digest:
                digests.extend(st.unit_digests((mid, up_real, up_mid), n))

        s.run_windows(args.window, consume if args.digest else None)
        per_rank = -(-s.total_units // s.world)
        row = {"elapsed_s": s.elapsed_local, "first_unit": float(s.start), "units": float(s.count),
               "numa_node": s.placement.get("numa_node"), "bound": 1.0 if s.placement.get("bound") else 0.0}
        if args.digest:
            row.update({f"sink_digest_{k:05d}": (float(digests[k]) if k < len(digests) else None) for k in range(per_rank)})
        rows = s.gather(row)
        out = s.summarize(rows)
        out.update(rank=s.rank, rows=rows, window=args.window,
                   placement={k: v for k, v in s.placement.items() if not k.startswith("_")})
        return out
    finally:
        s.close()


def stream_command(args, argv) -> int:
    """`stream`: started directly with --gpus N > 1 this process launches the N ranks as children (never an exec, never a HIP
    call here) and relays rank 0's JSON line; inside a rank (or with one GPU) it runs the rank's whole job (stream.run_sharded)."""
    import json

    from . import launch

    if args.gpus > 1 and not launch.under_launcher():
        rc, lines = launch.launch_ranks(args.gpus, "nu_scaler_amd.cli", argv, module=True)
        for ln in lines:
            print(ln, flush=True, file=sys.stdout if ln.startswith("{") else sys.stderr)
        return rc
    import os

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"nu_scaler_cli: error: --gpus {args.gpus} but WORLD_SIZE is {world}", file=sys.stderr)
        return 2
    from . import stream as S

    def sink(s):
        row = {}
        if args.host_fed_seconds > 0:
            row["host_fed_frames_per_s"] = s.run_host_fed(args.host_fed_seconds, algorithm=args.algorithm)
        if args.digest:
            per_rank = -(-s.total_units // s.world)  # every rank sends the same number of columns
            d = s.unit_digests()
            row.update({f"digest_{k:05d}": (float(d[k]) if k < len(d) else None) for k in range(per_rank)})
        return row or None

    if args.window > 0:
        out = _stream_in_windows(args, S)
    else:
        out = S.run_sharded(args.units * args.gpus, args.width, args.height, steps=args.steps, warmup=args.warmup,
                            source=S.SyntheticSource(args.pattern), sink=sink, backend=args.backend, bind=not args.no_bind,
                            force_device=args.force_device, schedule=args.schedule, algorithm=args.algorithm)
    if out["rank"] == 0:
        rows = out.pop("rows")
        if args.digest:
            digests = []
            for r in rows:
                digests += [int(r[k]) for k in sorted(r) if k.startswith("sink_digest_") and r[k] is not None]
            out["unit_digests"] = digests
        if args.host_fed_seconds > 0:
            rates = [r["sink_host_fed_frames_per_s"] for r in rows]
            out["host_fed_4k_frames_per_s"] = {"total": round(sum(rates), 1), "by_rank": [round(x, 1) for x in rates]}
        out["bound_by_rank"] = [bool(r["bound"]) for r in rows]
        out["numa_node_by_rank"] = [None if r["numa_node"] is None else int(r["numa_node"]) for r in rows]
        print(json.dumps(out), flush=True)
    return 0


def scene_line(cut: bool, sad: int, hist_l1: int, w: int, h: int) -> str:
    """The line `scene` prints: the flag and the two measures in the units of their thresholds (for reading; the decision
    itself is taken in integers on the device)."""
    return f"cut={1 if cut else 0} mad={sad / (3 * w * h):.3f} hist_permille={hist_l1 * 1000 / (2 * w * h):.1f}"


def _rate(text: str):
    """An integer or A/B -> Fraction; ValueError otherwise."""
    from fractions import Fraction

    parts = text.split("/")
    if len(parts) > 2 or not all(p.strip().isdigit() for p in parts):
        raise ValueError(f"a rate is an integer or a fraction A/B, got {text!r}")
    return Fraction(int(parts[0]), int(parts[1]) if len(parts) == 2 else 1)  # (a zero denominator raises ZeroDivisionError)


def _check_retime(args, parser) -> None:
    """Usage errors of `retime`: status 2 before anything is read or written."""
    from ._capi import FLOW_MAX_PROJECT, FLOW_MAX_WARPS
    from .imagefile import retime_output_paths
    from .retime import retime_ratio

    try:
        args.fps_in, args.fps_out = _rate(args.fps_in), _rate(args.fps_out)
        retime_ratio(args.fps_in, args.fps_out)
        retime_output_paths(args.output_pattern, 1)
    except (ValueError, ZeroDivisionError) as e:
        parser.error(str(e))
    if len(args.inputs) < 2:
        parser.error("retime needs at least 2 input frames")
    args.method = args.method.lower()
    if args.method not in ("optical_flow", "block_matching", "blend"):
        parser.error(f"--method must be optical_flow, block_matching or blend, got {args.method}")
    for name, v, ok in (("--flow-warps", args.flow_warps, range(FLOW_MAX_WARPS + 1)), ("--flow-median", args.flow_median, (0, 3, 5)),
                        ("--flow-project", args.flow_project, range(FLOW_MAX_PROJECT + 1))):
        if v is not None and args.method != "optical_flow":
            parser.error(f"{name} needs --method optical_flow")
        if v is not None and v not in ok:
            parser.error(f"{name}: {v} is out of range")
    if args.flow_bidirectional and args.method != "optical_flow":
        parser.error("--flow-bidirectional needs --method optical_flow")
    if args.bidirectional and args.method != "block_matching":
        parser.error("--bidirectional needs --method block_matching")


def _check_video(args, parser) -> None:
    """Usage errors of `video`: status 2 before anything is read or written."""
    from ._capi import FLOW_MAX_PROJECT, FLOW_MAX_WARPS, INTERP_MAX_TIMES

    if (args.fps_out is None) == (args.multiplier is None):
        parser.error("video needs --to or --multiplier, one of them")
    if args.fps_out is not None:
        try:
            args.fps_out = _rate(args.fps_out)
            if args.fps_out <= 0:
                raise ValueError(f"fps_out must be positive, got {args.fps_out!r}")
        except (ValueError, ZeroDivisionError) as e:
            parser.error(str(e))
    elif not 1 <= args.multiplier <= INTERP_MAX_TIMES + 1:
        parser.error(f"--multiplier must be from 1 to {INTERP_MAX_TIMES + 1}, got {args.multiplier}")
    args.method = args.method.lower()
    if args.method not in ("optical_flow", "block_matching", "blend"):
        parser.error(f"--method must be optical_flow, block_matching or blend, got {args.method}")
    for name, v, ok in (("--flow-warps", args.flow_warps, range(FLOW_MAX_WARPS + 1)), ("--flow-median", args.flow_median, (0, 3, 5)),
                        ("--flow-project", args.flow_project, range(FLOW_MAX_PROJECT + 1))):
        if v is not None and args.method != "optical_flow":
            parser.error(f"{name} needs --method optical_flow")
        if v is not None and v not in ok:
            parser.error(f"{name}: {v} is out of range")
    if args.flow_bidirectional and args.method != "optical_flow":
        parser.error("--flow-bidirectional needs --method optical_flow")
    if args.bidirectional and args.method != "block_matching":
        parser.error("--bidirectional needs --method block_matching")
    if not 1 <= args.scale <= 4:
        parser.error(f"--scale must be from 1 to 4, got {args.scale}")
    if args.matrix is not None and args.matrix.lower() not in ("bt601", "bt709"):
        parser.error(f"--matrix must be bt601 or bt709, got {args.matrix}")
    if args.window is not None and args.window < 2:
        parser.error(f"--window must be at least 2, got {args.window}")


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.command == "retime":
        _check_retime(args, parser)
    if args.command == "video":
        _check_video(args, parser)
        try:
            from .video import convert_y4m

            r = convert_y4m(args.input, args.output, fps_out=args.fps_out, multiplier=args.multiplier, method=args.method,
                            scale=args.scale, algorithm=args.algorithm, window_frames=args.window,
                            matrix=args.matrix.lower() if args.matrix else None, device=args.device, scene_detect=args.scene_detect,
                            flow_warps=args.flow_warps or 0, flow_median=args.flow_median or 0, flow_project=args.flow_project or 0,
                            bidirectional=args.bidirectional, flow_bidirectional=args.flow_bidirectional,
                            scale_domain=args.scale_domain)
            print(f"{args.output}: {r['frames_out']} frames {r['width']}x{r['height']} at {r['fps']} fps "
                  f"({r['frames_in']} read, {r['windows']} windows)")
        except (OSError, ValueError, RuntimeError) as e:
            print(f"nu_scaler_cli: error: {e}", file=sys.stderr)
            return 1
        return 0
    if args.command == "interpolate" and args.multiplier is not None:  # usage errors: status 2 before anything is read or written
        if args.t is not None:
            parser.error("--multiplier and --t exclude each other")
        from ._capi import INTERP_MAX_TIMES

        if not 2 <= args.multiplier <= INTERP_MAX_TIMES + 1:
            parser.error(f"--multiplier must be from 2 to {INTERP_MAX_TIMES + 1}, got {args.multiplier}")
    if args.command == "interpolate" and args.scene_detect and args.multiplier is None:
        parser.error("--scene-detect needs --multiplier")
    if args.command == "scene":
        if not 0 <= args.mad <= 255:
            parser.error(f"--mad must be from 0 to 255, got {args.mad}")
        if not 0 <= args.hist <= 1000:
            parser.error(f"--hist must be from 0 to 1000, got {args.hist}")
    if args.command == "interpolate" and args.method is not None:
        if args.flow:
            parser.error("--method and --flow exclude each other")
        if args.method.lower() != "block_matching":
            parser.error(f"--method must be block_matching, got {args.method}")
        if args.quality.lower() not in ("high", "medium", "low"):
            parser.error(f"--quality must be high, medium or low, got {args.quality}")
    if args.command == "interpolate" and args.flow_warps is not None:
        from ._capi import FLOW_MAX_WARPS

        if not args.flow:
            parser.error("--flow-warps needs --flow")
        if not 0 <= args.flow_warps <= FLOW_MAX_WARPS:
            parser.error(f"--flow-warps must be from 0 to {FLOW_MAX_WARPS}, got {args.flow_warps}")
    if args.command == "interpolate" and args.flow_median is not None:
        if not args.flow:
            parser.error("--flow-median needs --flow")
        if args.flow_median not in (0, 3, 5):
            parser.error(f"--flow-median must be 0, 3 or 5, got {args.flow_median}")
    if args.command == "interpolate" and args.flow_project is not None:
        if not args.flow:
            parser.error("--flow-project needs --flow")
        from ._capi import FLOW_MAX_PROJECT

        if not 0 <= args.flow_project <= FLOW_MAX_PROJECT:
            parser.error(f"--flow-project must be from 0 to {FLOW_MAX_PROJECT}, got {args.flow_project}")
    if args.command == "interpolate" and args.flow_bidirectional and not args.flow:
        parser.error("--flow-bidirectional needs --flow")
    if args.command == "interpolate":
        if (args.bidirectional or args.bidir_tolerance is not None) and args.method is None:
            parser.error("--bidirectional needs --method block_matching")
        if args.bidir_tolerance is not None:
            if not args.bidirectional:
                parser.error("--bidir-tolerance needs --bidirectional")
            if not 0 <= args.bidir_tolerance <= 96:
                parser.error(f"--bidir-tolerance must be from 0 to 96, got {args.bidir_tolerance}")
    if args.command == "stream":
        try:
            return stream_command(args, list(sys.argv[1:] if argv is None else argv))
        except (OSError, ValueError, RuntimeError) as e:
            print(f"nu_scaler_cli: error: {e}", file=sys.stderr)
            return 1
    from . import imagefile
    try:
        if args.command == "upscale":
            ow, oh = imagefile.upscale_image_file(args.input, args.output, args.tech, args.quality, args.scale,
                                                  args.algorithm, device=args.device)
            print(f"{args.output}: {ow}x{oh}")
        elif args.command == "retime":
            for path in imagefile.retime_image_files(args.output_pattern, args.inputs, args.fps_in, args.fps_out, args.method,
                                                     device=args.device, scene_detect=args.scene_detect,
                                                     bidirectional=args.bidirectional, flow_warps=args.flow_warps or 0,
                                                     flow_median=args.flow_median or 0, flow_project=args.flow_project or 0,
                                                     flow_bidirectional=args.flow_bidirectional):
                print(path)
        elif args.command == "compare":
            import numpy as np

            from .metrics import ErrorMetrics

            wa, ha, pa = imagefile.read_png(args.a)
            wb, hb, pb = imagefile.read_png(args.b)
            if (wa, ha) != (wb, hb):
                raise ValueError("Images must have the same dimensions")
            a = np.frombuffer(pa, np.uint8).reshape(ha, wa, 4)
            b = np.frombuffer(pb, np.uint8).reshape(hb, wb, 4)
            print(ErrorMetrics.calculate(a, b, device=args.device).line())
        elif args.command == "scene":
            from .scene import SceneDetector

            wa, ha, pa = imagefile.read_png(args.a)
            wb, hb, pb = imagefile.read_png(args.b)
            if (wa, ha) != (wb, hb):
                raise ValueError("Images must have the same dimensions")
            cut, sad, hist = SceneDetector(args.mad, args.hist, device=args.device).detect(pa, pb, wa, ha)
            print(scene_line(cut, sad, hist, wa, ha))
        elif args.method is not None:
            paths = imagefile.interpolate_image_files_block_matching(args.frame_a, args.frame_b, args.output, args.quality.lower(),
                                                                     0.5 if args.t is None else args.t, args.multiplier,
                                                                     device=args.device, scene_detect=args.scene_detect,
                                                                     bidirectional=args.bidirectional,
                                                                     tolerance=args.bidir_tolerance)
            for path in paths:
                print(path)
        elif args.multiplier is not None:
            for path in imagefile.interpolate_image_files_multi(args.frame_a, args.frame_b, args.output, args.multiplier, args.flow,
                                                                device=args.device, scene_detect=args.scene_detect,
                                                                flow_warps=args.flow_warps or 0, flow_median=args.flow_median or 0,
                                                                flow_project=args.flow_project or 0,
                                                                flow_bidirectional=args.flow_bidirectional):
                print(path)
        else:
            t = 0.5 if args.t is None else args.t
            w, h = imagefile.interpolate_image_files(args.frame_a, args.frame_b, args.output, t, args.flow, device=args.device,
                                                     flow_warps=args.flow_warps or 0, flow_median=args.flow_median or 0,
                                                     flow_project=args.flow_project or 0,
                                                     flow_bidirectional=args.flow_bidirectional)
            print(f"{args.output}: {w}x{h}")
    except (OSError, ValueError, RuntimeError) as e:
        print(f"nu_scaler_cli: error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
