"""Y4M video through the device-resident pipeline: `convert_y4m` reads planar 4:2:0 frames, converts them to RGBA8 on the device
(yuv.py), changes the frame rate on the route `retime.retime_frames` takes (flow estimator, block matcher or blend, scene cuts),
optionally up-scales every output frame, converts back and writes a Y4M file -- window by window, so that a clip of any length is
converted in bounded device memory.

The windows.  The schedule of a conversion by num / den (reduced; retime.py) repeats every `den` input frames: output j of a
window that starts at input frame f0, a multiple of den, is output f0 * num / den + j of the whole stream, with the same pair and
the same time.  So a window of m * den + 1 frames produces exactly the one-shot conversion's outputs; its last frame is a real
output that the next window, which starts there, produces again, and is kept only by the final window (`plan_windows`).
One window after the other: upload, compute and download do not overlap between windows."""
from __future__ import annotations

import ctypes
from fractions import Fraction
from math import gcd

from . import _capi as C

METHODS = ("optical_flow", "block_matching", "blend")
SCALE_DOMAINS = ("rgb", "yuv")
YUV_DOMAIN_ALGORITHMS = ("lanczos3", "lanczos", "bicubic", "catmullrom", "triangle")  # what yuv.YuvResizer resamples planes with


def plan_windows(n_frames: int, num: int, den: int, max_frames: int) -> list[tuple[int, int, int, int]]:
    """(first_frame, n_frames_in_window, first_output, n_outputs_kept) per window of a conversion of `n_frames` >= 2 frames by
    num / den with at most `max_frames` frames on the device at a time.  Every window starts at a multiple of the reduced den and
    holds m * den + 1 frames (m the largest that fits), except the last, which takes what is left; consecutive windows share one
    frame, whose output only the final window keeps -- so no window is ever left with that one frame alone.  ValueError for
    n_frames < 2, a term < 1 and max_frames < den + 1."""
    n_frames, num, den, max_frames = int(n_frames), int(num), int(den), int(max_frames)
    if num < 1 or den < 1:
        raise ValueError(f"the ratio {num}/{den} needs positive terms")
    g = gcd(num, den)
    num, den = num // g, den // g
    if n_frames < 2:
        raise ValueError("a stream needs at least 2 frames")
    if max_frames < den + 1:
        raise ValueError(f"a window needs at least den + 1 = {den + 1} frames for the ratio {num}/{den}, got {max_frames}")
    step = (max_frames - 1) // den * den
    out, first = [], 0
    while n_frames - first > step + 1:
        out.append((first, step + 1, first * num // den, step * num // den))
        first += step
    out.append((first, n_frames - first, first * num // den, (n_frames - 1 - first) * num // den + 1))
    return out


def default_matrix(height: int) -> str:
    """"bt709" from 720 rows up, else "bt601": what players assume of untagged video."""
    return "bt709" if int(height) >= 720 else "bt601"


def window_bytes_per_frame(w: int, h: int, num: int, den: int, scale: int, scale_domain: str = "rgb") -> int:
    """Device bytes one more input frame of a window costs: its I420 and RGBA forms, and num / den output frames in RGBA, in
    up-scaled RGBA (scale > 1) and in I420 (rounded up).  scale_domain "yuv" with scale > 1, the planar route: no up-scaled RGBA
    but an output's I420 form at the source size; at the ratio 1/1 only the frame's I420 form and the up-scaled one."""
    yuv_in, rgba_in = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2), w * h * 4
    ow, oh = w * scale, h * scale
    if scale_domain == "yuv" and scale > 1:
        yuv_out = ow * oh + 2 * ((ow + 1) // 2) * ((oh + 1) // 2)
        if num == den:
            return yuv_in + yuv_out
        return yuv_in + rgba_in + -(-(rgba_in + yuv_in + yuv_out) * num // den)
    per_out = rgba_in + (ow * oh * 4 if scale > 1 else 0) + ow * oh + 2 * ((ow + 1) // 2) * ((oh + 1) // 2)
    return yuv_in + rgba_in + -(-per_out * num // den)


def default_window_frames(w: int, h: int, num: int, den: int, scale: int, device: int = 0, scale_domain: str = "rgb") -> int:
    """The largest window whose frames -- input, RGBA input, RGBA output, up-scaled output and YUV output, or what the planar
    route holds instead (window_bytes_per_frame) -- use at most a quarter of the device's free memory (nus_device_memory_info),
    and at least den + 1.  (The estimators' flows and workspaces come on top; the other three quarters are theirs.)"""
    free, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
    if C.lib().nus_device_memory_info(int(device), ctypes.byref(free), ctypes.byref(total)) != C.OK:
        raise RuntimeError(C.last_error())
    return max(den + 1, int(free.value // 4 // window_bytes_per_frame(w, h, num, den, scale, scale_domain)))


def check_convert_args(fps_in, fps_out, multiplier, method, scale, bidirectional, *,
                       flow_bidirectional: bool = False, scale_domain: str = "rgb", algorithm: str = "lanczos3", width=None,
                       height=None) -> tuple[Fraction, int, int]:
    """The usage rules of `convert_y4m` that need no file and no device: (fps_out, num, den); ValueError otherwise.  With
    scale_domain "yuv" and scale > 1 the planes themselves are resampled: `algorithm` must be one of YUV_DOMAIN_ALGORITHMS, and
    `width` and `height` (where given: the clip's) even."""
    from .retime import retime_ratio

    if (fps_out is None) == (multiplier is None):
        raise ValueError("give fps_out or multiplier, one of them")
    if multiplier is not None:
        if isinstance(multiplier, bool) or not isinstance(multiplier, int) or not 1 <= multiplier <= C.INTERP_MAX_TIMES + 1:
            raise ValueError(f"multiplier must be an integer from 1 to {C.INTERP_MAX_TIMES + 1}, got {multiplier!r}")
        fps_out = Fraction(fps_in) * multiplier
    fps_out = Fraction(fps_out)
    num, den = retime_ratio(Fraction(fps_in), fps_out)
    if method not in METHODS:
        raise ValueError(f"method must be optical_flow, block_matching or blend, got {method}")
    if bidirectional and method != "block_matching":
        raise ValueError("bidirectional needs method block_matching")
    if flow_bidirectional and method != "optical_flow":
        raise ValueError("flow_bidirectional needs method optical_flow")
    if isinstance(scale, bool) or not isinstance(scale, int) or not 1 <= scale <= 4:
        raise ValueError(f"scale must be an integer from 1 to 4, got {scale!r}")
    if scale_domain not in SCALE_DOMAINS:
        raise ValueError(f"scale_domain must be 'rgb' or 'yuv', got {scale_domain!r}")
    if scale_domain == "yuv" and scale > 1:
        if not isinstance(algorithm, str) or algorithm.lower() not in YUV_DOMAIN_ALGORITHMS:
            raise ValueError(f"scale_domain 'yuv' resamples the Y, U and V planes with lanczos3, bicubic or triangle, not with "
                             f"{algorithm!r}: nearest, bilinear and the FSR algorithms need scale_domain 'rgb'")
        if (width is not None and int(width) % 2) or (height is not None and int(height) % 2):
            raise ValueError(f"scale_domain 'yuv' needs an even width and height (the chroma planes must be exactly half the luma "
                             f"planes), got {width}x{height}: odd sizes need scale_domain 'rgb'")
    return fps_out, num, den


class _Route:
    """The handles of one conversion and the device-resident retime of a window: `retime.retime_frames`' route without its upload
    and download."""

    def __init__(self, method, device, scene_detect, flow_warps, flow_median, flow_project, bidirectional,
                 flow_bidirectional: bool = False):
        self.matcher = self.warp = self.flow = self.scene = None
        self.select = bool(flow_bidirectional) and method == "optical_flow"  # both flows of every pair and the select warp
        if method == "block_matching":
            from .blockmatch import BlockMatcher

            self.matcher = BlockMatcher("medium", device=device, bidirectional=bidirectional)
            if scene_detect:
                self.matcher.set_scene_detect(True)
        else:
            from .interpolator import WgpuFrameInterpolator
            from .scene import SceneDetector

            self.warp = WgpuFrameInterpolator(device=device)
            if method == "optical_flow":
                from .flow import FlowEstimator

                self.flow = FlowEstimator(device=device, warps=flow_warps, median=flow_median)
                if flow_project:
                    self.warp.set_flow_project(flow_project)
            self.scene = SceneDetector(device=device) if scene_detect else None

    def retime(self, torch, dev, d_in: int, n: int, w: int, h: int, num: int, den: int, d_out: int, s: int) -> list:
        """Enqueue the conversion of the n RGBA frames at d_in (tight) into d_out (tight) on stream s; returns the tensors that
        must stay alive until the stream has run."""
        fb = w * h * 4
        keep = []

        def scratch(nbytes):  # 16-byte aligned device bytes
            t = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)
            keep.append(t)
            return (t.data_ptr() + 15) & ~15

        if self.matcher is not None:
            ws_bytes = self.matcher.stream_workspace_size(w, h, n)
            self.matcher.retime_stream_device(d_in, fb, n, w, h, num, den, scratch(ws_bytes), ws_bytes, d_out, stream=s)
            return keep
        d_flows = 0
        if self.select:
            flows = torch.empty((2, n - 1, h, w, 2), dtype=torch.float32, device=dev)
            keep.append(flows)
            self.flow.estimate_both_device_stream(d_in, n, w, h, flows[0].data_ptr(), flows[1].data_ptr(), s)
            self.warp.retime_select_device(d_in, fb, n, flows[0].data_ptr(), flows[1].data_ptr(), w, h, num, den, d_out, 0, s)
        else:
            if self.flow is not None:
                flows = torch.empty((n - 1, h, w, 2), dtype=torch.float32, device=dev)
                keep.append(flows)
                self.flow.estimate_device_stream(d_in, n, w, h, flows.data_ptr(), s)
                d_flows = flows.data_ptr()
            self.warp.retime_device(d_in, fb, n, d_flows, w, h, num, den, d_out, 0, s)
        if self.scene is not None:
            ws_bytes = self.scene.workspace_size(w, h, n - 1)
            d_ws, d_cut = scratch(ws_bytes), scratch(n - 1)
            self.scene.detect_device(d_in, fb, d_in + fb, fb, w, h, n - 1, d_ws, ws_bytes, d_cut, stream=s)
            if C.lib().nus_scene_apply_cuts_retime_device(d_in, fb, n, w, h, C.FORMAT_RGBA8, num, den, d_cut, d_out, 0, s) != C.OK:
                raise RuntimeError(C.last_error())
        return keep


def convert_y4m(in_path, out_path, *, fps_out=None, multiplier=None, method: str = "optical_flow", scale: int = 1,
                algorithm: str = "lanczos3", window_frames=None, matrix=None, device: int = 0, scene_detect: bool = False,
                flow_warps: int = 0, flow_median: int = 0, flow_project: int = 0, bidirectional: bool = False,
                flow_bidirectional: bool = False, scale_domain: str = "rgb") -> dict:
    """IN.y4m at its rate -> OUT.y4m at `fps_out` (an int or a Fraction) or at `multiplier` times the input's rate, every output
    frame `scale` times as large with `algorithm` when scale > 1.  method "optical_flow" (Horn-Schunck, the estimator's defaults,
    with flow_warps / flow_median / flow_project; `flow_bidirectional`: both flows of every pair and the select warp), "block_matching" (the Medium preset; `bidirectional`: its forward-backward
    check) or "blend" (zero flow); `scene_detect`: repeats instead of blends across a cut.  matrix "bt601" | "bt709" (None: by the
    input's height); the range and the chroma siting are the input's, the chroma is up-sampled bilinearly.  window_frames: input
    frames on the device at a time (None: from the device's free memory), at least den + 1 of the reduced ratio.  The output
    header carries W * scale, H * scale, F = fps_out reduced and the input's I, A, C and XCOLORRANGE tags.
    scale_domain "rgb" (default): every output frame is up-scaled as RGBA8 and converted to I420 at the target size.  "yuv" (with
    scale > 1; lanczos3, bicubic or triangle; even sizes): the output frames are converted to I420 at the SOURCE size and their Y, U
    and V planes up-scaled themselves (yuv.YuvResizer, chroma at the input's siting); at the ratio 1/1 (e.g. multiplier=1) nothing is
    converted at all -- upload, plane up-scale, download -- and `method` is not consulted.
    Returns {"frames_in", "frames_out", "windows", "width", "height", "fps"}.  ValueError for what is refused."""
    import torch

    from . import transfer, yuv
    from .y4m import Y4MReader, Y4MWriter

    with Y4MReader(in_path) as rd:
        fps_out, num, den = check_convert_args(rd.fps, fps_out, multiplier, method, scale, bidirectional,
                                                flow_bidirectional=flow_bidirectional, scale_domain=scale_domain, algorithm=algorithm,
                                                width=rd.width, height=rd.height)
        w, h = rd.width, rd.height
        planar = scale_domain == "yuv" and scale > 1
        direct = planar and num == den  # up-scaling only: no colour conversion, no estimator
        ow, oh = w * scale, h * scale
        if matrix is None:
            matrix = default_matrix(h)
        fmt = yuv.YuvFormat(matrix=matrix, range=rd.range, siting=rd.siting, chroma="bilinear")
        if window_frames is None:
            window_frames = default_window_frames(w, h, num, den, scale, device, scale_domain)
        window_frames = int(window_frames)
        if window_frames < den + 1:
            raise ValueError(f"a window needs at least den + 1 = {den + 1} frames for the ratio {num}/{den}, got {window_frames}")
        step = (window_frames - 1) // den * den
        route = None if direct else _Route(method, device, scene_detect, flow_warps, flow_median, flow_project, bidirectional,
                                           flow_bidirectional)
        up = planes = None
        if planar:
            planes = yuv.YuvResizer(w, h, ow, oh, algorithm=algorithm, siting=rd.siting, mode="fma", device=device)
        elif scale > 1:
            from .upscaler import PyWgpuUpscaler

            up = PyWgpuUpscaler("quality", algorithm, device=device)
            up.initialize(w, h, ow, oh)
        yb_in, yb_out, fb = yuv.frame_bytes(w, h), yuv.frame_bytes(ow, oh), w * h * 4
        dev = f"cuda:{int(device)}"
        x_range = [t for t in rd.x_tags if t.startswith("COLORRANGE=")]
        frames_in = frames_out = windows = 0
        with torch.cuda.device(dev), Y4MWriter(out_path, ow, oh, fps_out, rd.siting, None, rd.aspect, rd.interlace, rd.colorspace,
                                               x_range) as wr:
            s = torch.cuda.current_stream().cuda_stream
            # plan_windows' plan, walked without knowing the clip's length: one frame read ahead of the window tells whether it is
            # the final one; a window's last frame opens the next
            frames = rd.read_frames(step + 2)
            if len(frames) < 2:
                raise ValueError(f"{in_path}: a conversion needs at least 2 frames, the file holds {len(frames)}")
            frames_in = len(frames)
            while True:
                final = len(frames) <= step + 1
                win = frames if final else frames[:step + 1]
                n = len(win)
                n_out = (n - 1) * num // den + 1
                kept = n_out if final else n_out - 1
                d_yuv = torch.empty((n, yb_in), dtype=torch.uint8, device=dev)
                for k, f in enumerate(win):
                    transfer.upload(d_yuv[k].data_ptr(), f, s)
                if direct:
                    d_res = torch.empty((kept, yb_out), dtype=torch.uint8, device=dev)
                    planes.resize_device(d_yuv.data_ptr(), d_res.data_ptr(), kept, stream=s)
                    res = transfer.to_numpy(d_res)
                    for j in range(kept):
                        wr.write(res[j])
                    del d_yuv, d_res
                    frames_out += kept
                    windows += 1
                    if final:
                        break
                    more = rd.read_frames(step)
                    frames_in += len(more)
                    frames = frames[step:] + more
                    continue
                d_in = torch.empty((n, fb), dtype=torch.uint8, device=dev)
                yuv.to_rgba_device(d_yuv.data_ptr(), w, h, d_in.data_ptr(), fmt, n, stream=s)
                d_out = torch.empty((n_out, fb), dtype=torch.uint8, device=dev)
                keep = route.retime(torch, dev, d_in.data_ptr(), n, w, h, num, den, d_out.data_ptr(), s)
                d_big = d_out
                if up is not None:
                    d_big = torch.empty((kept, ow * oh * 4), dtype=torch.uint8, device=dev)
                    up.upscale_device(d_out.data_ptr(), d_big.data_ptr(), kept, s)
                d_res = torch.empty((kept, yb_out), dtype=torch.uint8, device=dev)
                if planes is not None:  # to I420 at the source size, then the planes themselves: no target-size RGBA
                    d_big = torch.empty((kept, yb_in), dtype=torch.uint8, device=dev)
                    yuv.to_yuv_device(d_out.data_ptr(), w, h, d_big.data_ptr(), fmt, kept, stream=s)
                    planes.resize_device(d_big.data_ptr(), d_res.data_ptr(), kept, stream=s)
                else:
                    yuv.to_yuv_device(d_big.data_ptr(), ow, oh, d_res.data_ptr(), fmt, kept, stream=s)
                res = transfer.to_numpy(d_res)  # (ordered after the stream's work; returns when the bytes are on the host)
                for j in range(kept):
                    wr.write(res[j])
                del keep, d_yuv, d_in, d_out, d_big, d_res
                frames_out += kept
                windows += 1
                if final:
                    break
                more = rd.read_frames(step)
                frames_in += len(more)
                frames = frames[step:] + more
    return {"frames_in": frames_in, "frames_out": frames_out, "windows": windows, "width": ow, "height": oh, "fps": fps_out}
