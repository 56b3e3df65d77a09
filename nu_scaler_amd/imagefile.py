"""Image-file front end of the upscaler: `upscale_image_file` as in the legacy crate
(Nu_scale/src/upscale/mod.rs:307-338 and :341-356) plus the matching interpolation helper.

The reference decodes with the `image` crate and converts to RGBA8 (`image::open(..)?.to_rgba8()`);
here a small PNG codec (8-bit, non-interlaced, colour types 0/2/3/4/6) on zlib + numpy does that,
because nothing else in the image can read PNGs.  Pixels go through the HIP path only
(`PyWgpuUpscaler` / `WgpuFrameInterpolator`): no CPU resampling here.
"""
from __future__ import annotations

import os
import struct
import zlib

from .interpolator import WgpuFrameInterpolator
from .upscaler import PyWgpuUpscaler

_SIG = b"\x89PNG\r\n\x1a\n"


def _np():
    import numpy as np
    return np


def _unfilter(raw: bytes, w: int, h: int, bpp: int):
    """Undo the five PNG row filters (PNG spec section 9).  bpp = bytes per complete pixel."""
    np = _np()
    stride = w * bpp
    if len(raw) < h * (stride + 1):
        raise ValueError("PNG: truncated image data")
    rows = np.frombuffer(raw, np.uint8, h * (stride + 1)).reshape(h, stride + 1)
    out = np.empty((h, stride), np.uint8)
    zero = np.zeros(stride, np.uint8)
    for y in range(h):
        ft = int(rows[y, 0])
        line = rows[y, 1:]
        prev = out[y - 1] if y else zero
        if ft == 0:
            out[y] = line
        elif ft == 1:  # Sub: running sum per channel, modulo 256
            out[y] = np.cumsum(line.reshape(w, bpp), axis=0, dtype=np.uint8).reshape(stride)
        elif ft == 2:  # Up
            out[y] = line + prev
        elif ft in (3, 4):  # Average / Paeth: sequential along the row, vectorised over the pixel's bytes
            cur = np.zeros((w + 1, bpp), np.int32)  # cur[0] = the zero pixel left of the row
            up = np.zeros((w + 1, bpp), np.int32)
            up[1:] = prev.reshape(w, bpp)
            ln = line.reshape(w, bpp).astype(np.int32)
            if ft == 3:
                for x in range(w):
                    cur[x + 1] = (ln[x] + ((cur[x] + up[x + 1]) >> 1)) & 255
            else:
                for x in range(w):
                    a, b, c = cur[x], up[x + 1], up[x]
                    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
                    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
                    cur[x + 1] = (ln[x] + pred) & 255
            out[y] = cur[1:].astype(np.uint8).reshape(stride)
        else:
            raise ValueError(f"PNG: unknown filter type {ft}")
    return out


def read_png(path: str):
    """-> (width, height, RGBA8 bytes), what `image::open(path)?.to_rgba8()` yields for 8-bit PNGs."""
    np = _np()
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _SIG:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, hdr, palette, trns = 8, [], None, None, None
    while pos + 8 <= len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"PLTE":
            palette = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif typ == b"tRNS":
            trns = np.frombuffer(body, np.uint8)
        elif typ == b"IDAT":
            idat.append(body)
        elif typ == b"IEND":
            break
    if hdr is None:
        raise ValueError(f"{path}: PNG without IHDR")
    w, h, depth, ctype, _, _, interlace = hdr
    if depth != 8 or interlace != 0 or ctype not in (0, 2, 3, 4, 6):
        raise ValueError(f"{path}: unsupported PNG flavour (depth {depth}, colour type {ctype}, interlace {interlace})")
    ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    px = _unfilter(zlib.decompress(b"".join(idat)), w, h, ch).reshape(h, w, ch)
    rgba = np.full((h, w, 4), 255, np.uint8)
    if ctype == 6:
        rgba = px
    elif ctype == 2:
        rgba[..., :3] = px
    elif ctype == 0:
        rgba[..., :3] = px
    elif ctype == 4:
        rgba[..., :3] = px[..., :1]
        rgba[..., 3] = px[..., 1]
    else:
        if palette is None:
            raise ValueError(f"{path}: palette PNG without PLTE")
        rgba[..., :3] = palette[px[..., 0]]
        if trns is not None:
            alpha = np.full(256, 255, np.uint8)
            alpha[:len(trns)] = trns
            rgba[..., 3] = alpha[px[..., 0]]
    return w, h, np.ascontiguousarray(rgba).tobytes()


def write_png(path: str, width: int, height: int, rgba: bytes) -> None:
    """8-bit RGBA, filter 0 on every row."""
    np = _np()
    if len(rgba) != width * height * 4:
        raise ValueError("write_png: buffer size does not match width * height * 4")
    rows = np.zeros((height, width * 4 + 1), np.uint8)
    rows[:, 1:] = np.frombuffer(rgba, np.uint8).reshape(height, width * 4)

    def chunk(typ: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(_SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


# quality -> algorithm when none is given (Nu_scale/src/upscale/mod.rs:295-303)
_QUALITY_TO_ALGORITHM = {"ultra": "lanczos3", "quality": "bicubic", "balanced": "bicubic", "performance": "bilinear"}


def output_size(width: int, height: int, scale_factor: float):
    """`(input_width as f32 * scale_factor) as u32` (Nu_scale/src/upscale/mod.rs:320-321)."""
    np = _np()
    s = np.float32(scale_factor)
    return int(np.float32(width) * s), int(np.float32(height) * s)


def upscale_image_file(input_path: str, output_path: str, technology: str = "fallback", quality: str = "quality",
                       scale_factor: float = 2.0, algorithm: str | None = None, device: int = 0) -> tuple[int, int]:
    """Nu_scale/src/upscale/mod.rs:307-338: load, upscale, save.  Returns the output size.

    `technology`: "fallback" (the algorithm menu), "fsr" (the FSR1-style pass pair), "none"
    (pass-through copy, as PassThroughUpscaler).  "dlss" has no equivalent on this hardware and is an
    error rather than a silent substitute.
    """
    w, h, px = read_png(input_path)
    tech = str(technology).lower()
    if tech == "none":
        write_png(output_path, w, h, px)
        return w, h
    if tech == "dlss":
        raise ValueError("technology 'dlss' is not available on this device")
    if tech not in ("fallback", "fsr", "wgpu"):
        raise ValueError(f"unknown technology '{technology}'")
    ow, oh = output_size(w, h, scale_factor)
    if ow == 0 or oh == 0:
        raise ValueError("scale factor gives an empty output image")
    if tech == "fsr":
        alg = "fsr1"
    else:
        alg = (algorithm or _QUALITY_TO_ALGORITHM.get(str(quality).lower(), "bicubic")).lower()
    up = PyWgpuUpscaler(quality, alg, device=device)
    up.initialize(w, h, ow, oh)
    write_png(output_path, ow, oh, up.upscale(px))
    return ow, oh


def _check_flow_warps(flow_warps, estimate_flow: bool) -> int:
    from .flow import check_warps

    flow_warps = check_warps(flow_warps)
    if flow_warps and not estimate_flow:
        raise ValueError("flow_warps needs estimate_flow (--flow-warps needs --flow)")
    return flow_warps


def _check_flow_median(flow_median, estimate_flow: bool) -> int:
    from .flow import check_median

    flow_median = check_median(flow_median)
    if flow_median and not estimate_flow:
        raise ValueError("flow_median needs estimate_flow (--flow-median needs --flow)")
    return flow_median


def _check_flow_project(flow_project, estimate_flow: bool) -> int:
    from .flow import check_project

    flow_project = check_project(flow_project)
    if flow_project and not estimate_flow:
        raise ValueError("flow_project needs estimate_flow (--flow-project needs --flow)")
    return flow_project


def _check_flow_bidirectional(flow_bidirectional, estimate_flow: bool) -> None:
    if flow_bidirectional and not estimate_flow:
        raise ValueError("flow_bidirectional needs estimate_flow (--flow-bidirectional needs --flow)")


def interpolate_image_files(path_a: str, path_b: str, output_path: str, time_t: float = 0.5, estimate_flow: bool = False,
                            device: int = 0, flow_warps: int = 0, flow_median: int = 0, flow_project: int = 0,
                            flow_bidirectional: bool = False) -> tuple[int, int]:
    """The in-between frame of two equally sized images (wgpu_interpolator.rs:215-491); with
    `estimate_flow` the Horn-Schunck front end supplies the motion field (`flow_warps`: its re-linearisation rounds per finer
    level, FlowEstimator.set_warps; `flow_median`: its median filter behind every Jacobi run, 0, 3 or 5, FlowEstimator.set_median;
    `flow_project`: projection rounds of the warp with that field, WgpuFrameInterpolator.set_flow_project; `flow_bidirectional`:
    the flow is estimated both ways and each pixel takes the vector whose two samples agree better,
    WgpuFrameInterpolator.interpolate_select_py), otherwise zero flow as the reference's live path."""
    _check_flow_bidirectional(flow_bidirectional, estimate_flow)
    flow_warps = _check_flow_warps(flow_warps, estimate_flow)
    flow_median = _check_flow_median(flow_median, estimate_flow)
    flow_project = _check_flow_project(flow_project, estimate_flow)
    w, h, a = read_png(path_a)
    wb, hb, b = read_png(path_b)
    if (w, h) != (wb, hb):
        raise ValueError(f"frame sizes differ: {w}x{h} vs {wb}x{hb}")
    it = WgpuFrameInterpolator(device=device)
    if flow_project:
        it.set_flow_project(flow_project)
    flow = None
    if estimate_flow:
        from .flow import FlowEstimator
        fe = FlowEstimator(device=device, warps=flow_warps, median=flow_median)
        flow = fe.estimate(a, b, w, h)
    if flow is not None and flow_bidirectional:
        out = it.interpolate_select_py(a, b, w, h, flow, fe.estimate(b, a, w, h), time_t=time_t)
    else:
        out = it.interpolate_py(a, b, w, h, time_t=time_t, flow=flow) if flow is not None else it.interpolate_py(a, b, w, h, time_t=time_t)
    write_png(output_path, w, h, out)
    return w, h


def multi_output_paths(output_path: str, multiplier: int) -> list[str]:
    """Where `interpolate --multiplier M` writes its M - 1 frames: <stem>_<k><ext> for k = 1 .. M - 1."""
    stem, ext = os.path.splitext(output_path)
    return [f"{stem}_{k}{ext}" for k in range(1, int(multiplier))]


def interpolate_image_files_multi(path_a: str, path_b: str, output_path: str, multiplier: int, estimate_flow: bool = False,
                                  device: int = 0, scene_detect: bool = False, flow_warps: int = 0, flow_median: int = 0,
                                  flow_project: int = 0, flow_bidirectional: bool = False) -> list[str]:
    """The M - 1 in-between frames of a frame-rate multiplier M (t = k / M) from one multi-time call, written to
    multi_output_paths(output_path, M); with `estimate_flow` the flow is estimated once for all of them.  `scene_detect`: a
    pair the scene-cut detector flags gives repeats of the nearer frame instead of blends.  `flow_bidirectional`: both flows and
    the select warp, as interpolate_image_files."""
    from .interpolator import frame_times

    _check_flow_bidirectional(flow_bidirectional, estimate_flow)
    flow_warps = _check_flow_warps(flow_warps, estimate_flow)
    flow_median = _check_flow_median(flow_median, estimate_flow)
    flow_project = _check_flow_project(flow_project, estimate_flow)
    times = frame_times(multiplier)
    w, h, a = read_png(path_a)
    wb, hb, b = read_png(path_b)
    if (w, h) != (wb, hb):
        raise ValueError(f"frame sizes differ: {w}x{h} vs {wb}x{hb}")
    it = WgpuFrameInterpolator(device=device)
    if flow_project:
        it.set_flow_project(flow_project)
    flow = None
    if estimate_flow:
        from .flow import FlowEstimator
        fe = FlowEstimator(device=device, warps=flow_warps, median=flow_median)
        flow = fe.estimate(a, b, w, h)
    cut = False
    if flow is not None and flow_bidirectional and scene_detect:
        from .scene import SceneDetector

        cut = SceneDetector(device=device).detect(a, b, w, h)[0]
    if flow is not None and flow_bidirectional and not cut:
        frames = it.interpolate_select_multi_py(a, b, w, h, flow, fe.estimate(b, a, w, h), times=times)
    else:
        frames = it.interpolate_multi_py(a, b, w, h, times=times, flow=flow, scene_detect=scene_detect)
    paths = multi_output_paths(output_path, multiplier)
    for path, out in zip(paths, frames):
        write_png(path, w, h, out)
    return paths


def interpolate_image_files_block_matching(path_a: str, path_b: str, output_path: str, quality: str = "medium",
                                           time_t: float = 0.5, multiplier: int | None = None, device: int = 0,
                                           scene_detect: bool = False, bidirectional: bool = False,
                                           tolerance: int | None = None) -> list[str]:
    """`interpolate --method block_matching`: the block matcher's vectors (preset of `quality`; with `bidirectional` after the
    forward-backward check at `tolerance`, None: the default) drive the warp.  One frame at
    `time_t` written to output_path, or with `multiplier` the M - 1 frames at multi_output_paths(output_path, M).  Returns the
    paths written."""
    from .blockmatch import BlockMatcher

    w, h, a = read_png(path_a)
    wb, hb, b = read_png(path_b)
    if (w, h) != (wb, hb):
        raise ValueError(f"frame sizes differ: {w}x{h} vs {wb}x{hb}")
    bm = BlockMatcher(quality, device=device)
    if bidirectional:
        bm.set_bidirectional(True) if tolerance is None else bm.set_bidirectional(True, tolerance)
    if scene_detect:
        bm.set_scene_detect(True)
    if multiplier is not None:
        frames, paths = bm.interpolate(a, b, w, h, multiplier=multiplier), multi_output_paths(output_path, multiplier)
    else:
        frames, paths = bm.interpolate(a, b, w, h, times=[time_t]), [output_path]
    for path, out in zip(paths, frames):
        write_png(path, w, h, out)
    return paths


def retime_output_paths(pattern: str, n_out: int) -> list[str]:
    """`pattern % j` for every output frame j; ValueError unless the pattern holds exactly one integer conversion (OUT_%04d.png)."""
    import re

    if len(re.findall(r"%0?\d*d", pattern)) != 1 or pattern.replace("%%", "").count("%") != 1:
        raise ValueError(f"the output pattern needs exactly one %d conversion (as OUT_%04d.png), got {pattern!r}")
    return [pattern % j for j in range(n_out)]


def retime_image_files(output_pattern: str, input_paths, fps_in, fps_out, method: str = "optical_flow", *, device: int = 0,
                       scene_detect: bool = False, bidirectional: bool = False, flow_warps: int = 0, flow_median: int = 0,
                       flow_project: int = 0, flow_bidirectional: bool = False) -> list[str]:
    """PNG frames at `fps_in` -> PNG frames at `fps_out`, written to `output_pattern % j` (retime.py has the schedule): method
    "optical_flow" (Horn-Schunck, the estimator's defaults), "block_matching" (the Medium preset) or "blend" (zero flow).
    `flow_bidirectional` (optical_flow only): every pair's flow is estimated both ways and each pixel takes the vector whose two
    samples agree better (retime_frames' `select`).  Returns the paths written."""
    if flow_bidirectional and method != "optical_flow":
        raise ValueError("flow_bidirectional needs method optical_flow")
    import torch  # noqa: F401  (the device buffers are torch's: its HIP runtime has to be loaded before the library loads its own)

    from .retime import retime_count, retime_frames

    paths = retime_output_paths(output_pattern, retime_count(len(input_paths), fps_in, fps_out))
    images = [read_png(p) for p in input_paths]
    w, h = images[0][0], images[0][1]
    if any((iw, ih) != (w, h) for iw, ih, _ in images):
        raise ValueError("Images must have the same dimensions")
    frames = [px for _, _, px in images]
    if method == "block_matching":
        from .blockmatch import BlockMatcher

        bm = BlockMatcher("medium", device=device, bidirectional=bidirectional)
        if scene_detect:
            bm.set_scene_detect(True)
        out = retime_frames(frames, w, h, fps_in, fps_out, matcher=bm, device=device)
    else:
        from .interpolator import WgpuFrameInterpolator
        from .scene import SceneDetector

        flow = None
        warp = WgpuFrameInterpolator(device=device)
        if method == "optical_flow":
            from .flow import FlowEstimator

            flow = FlowEstimator(device=device, warps=flow_warps, median=flow_median)
            if flow_project:
                warp.set_flow_project(flow_project)
        scene = SceneDetector(device=device) if scene_detect else None
        out = retime_frames(frames, w, h, fps_in, fps_out, warp=warp, flow=flow, scene=scene, device=device,
                            select=bool(flow_bidirectional))
    for path, px in zip(paths, out):
        write_png(path, w, h, px)
    return paths
