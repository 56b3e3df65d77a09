"""Optical-flow front end of the frame interpolator ("next" row).

Mirrors the reference's `WgpuFrameInterpolator::build_pyramid` / `compute_coarse_flow`
(nu_scaler_core/src/wgpu_interpolator.rs:969-1203): Gaussian pyramid (5-tap blur H/V + 2x box
downsample) of both frames, Horn-Schunck Jacobi steps at the coarsest level, then -- where the
reference's refine path is dead code -- a coarse-to-fine warm start: x2 bilinear flow upsample
and more Jacobi steps per finer level.  The result is the dense (dx, dy) field that
`WgpuFrameInterpolator.interpolate_py(..., flow=...)` consumes.  With `warps=N` (off by default) every finer level is
re-linearised N times about the flow it has -- frame B sampled through it -- which is what follows motion of more than a pixel.
With `median=3` or `5` (off by default; meant for `warps >= 1`) the level's flow is median-filtered after every Jacobi run, which
keeps motion boundaries from turning into ramps.  With `project=N` (off by default) the warp behind the estimator evaluates the
flow at the in-between time: every output pixel looks its vector up where its content came from before it is warped.
With `bidirectional=True` (off by default) the stream interpolation estimates every pair both ways and each output pixel takes the
forward or the backward vector, whichever makes its two samples agree better (the select warp).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi as C


def check_warps(warps) -> int:
    """`warps` as an int in 0 .. FLOW_MAX_WARPS, or ValueError (what every Python entry point that takes the setting shares)."""
    if isinstance(warps, bool) or int(warps) != warps:
        raise ValueError(f"flow warps must be an integer from 0 to {C.FLOW_MAX_WARPS}, got {warps!r}")
    if not 0 <= int(warps) <= C.FLOW_MAX_WARPS:
        raise ValueError(f"flow warps must be from 0 to {C.FLOW_MAX_WARPS}, got {warps}")
    return int(warps)


MEDIAN_SIZES = (0, 3, 5)  # what nus_flow_set_median takes (0: off)


def check_median(size) -> int:
    """`size` as one of MEDIAN_SIZES, or ValueError (what every Python entry point that takes the setting shares)."""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or int(size) not in MEDIAN_SIZES:
        raise ValueError(f"flow median must be 0 (off), 3 or 5, got {size!r}")
    return int(size)


def check_project(rounds) -> int:
    """`rounds` (projection rounds of the dense-flow warp) as an int in 0 .. FLOW_MAX_PROJECT, or ValueError (what every Python
    entry point that takes the setting shares)."""
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or not 0 <= int(rounds) <= C.FLOW_MAX_PROJECT:
        raise ValueError(f"flow projection rounds must be an integer from 0 to {C.FLOW_MAX_PROJECT}, got {rounds!r}")
    return int(rounds)


class FlowEstimator:
    def __init__(self, levels: int = 3, coarse_iterations: int = 50, refine_iterations: int = 10,
                 lambda_: float = 0.02 ** 2, *, device: int = 0, warps: int = 0, median: int = 0, project: int = 0,
                 bidirectional: bool = False):
        # lambda default: the value of the reference's own (ignored) test, wgpu_interpolator.rs:1535
        self._lib = C.lib()
        self._h = self._lib.nus_flow_create()
        if not self._h:
            raise RuntimeError(C.last_error())
        self.levels, self.coarse_iterations = int(levels), int(coarse_iterations)
        self.refine_iterations, self.lambda_ = int(refine_iterations), float(lambda_)
        self._check(self._lib.nus_flow_set_device(self._h, int(device)))
        if warps != 0:
            self.set_warps(warps)
        if median != 0:
            self.set_median(median)
        if project != 0:
            self.set_project(project)
        if bidirectional:
            self.set_bidirectional(True)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.nus_flow_destroy(h)

    def set_tiled(self, enabled) -> None:
        """True / 1 (default): multi-step Horn-Schunck kernels (2: always LDS tiles, 3: always the
        register-pipelined kernel); False / 0: one plain kernel per step.  Same bits either way."""
        self._check(self._lib.nus_flow_set_tiled(self._h, int(enabled)))

    def set_mode(self, mode: str) -> None:
        """"exact" (default): every stage bit-identical to the oracle; "fast": the estimators' Jacobi steps in separable sums,
        reciprocals and FMAs (flow within 1e-3 px; with warps see nus_flow_set_mode)."""
        m = {"exact": 0, "fast": 1}.get(str(mode).lower())
        if m is None:
            raise ValueError("mode must be 'exact' or 'fast'")
        self._check(self._lib.nus_flow_set_mode(self._h, m))

    def set_warps(self, warps: int) -> None:
        """Re-linearisation rounds per finer pyramid level (nus_flow_set_warps; 0, the default, .. FLOW_MAX_WARPS): each round samples
        frame B through the level's current flow and runs the level's Jacobi steps on the residual equation about that flow, so the
        estimate follows motion of more than a pixel.  Applies to every estimator entry point of this object."""
        w = check_warps(warps)
        self._check(self._lib.nus_flow_set_warps(self._h, w))

    @property
    def warps(self) -> int:
        return int(self._lib.nus_flow_warps(self._h))

    def set_median(self, size: int) -> None:
        """Median filter of the flow behind every Jacobi run (nus_flow_set_median; 0, the default, is off; 3 or 5 is the window):
        after the coarsest level's steps, a finer level's steps and each re-linearisation round the level's flow is replaced by its
        component-wise size x size median (border replicated).  Meant for `warps >= 1` (with warps = 0 the result is mixed); small
        frames want 3.  Applies to every estimator entry point of this object."""
        s = check_median(size)
        self._check(self._lib.nus_flow_set_median(self._h, s))

    @property
    def median_size(self) -> int:
        return int(self._lib.nus_flow_median_size(self._h))

    def set_project(self, rounds: int) -> None:
        """Projection rounds of the warp behind the estimator (nus_flow_set_project; 0, the default, is off; at most
        FLOW_MAX_PROJECT): `interpolate_device_stream` and `interpolate_multi_device_stream` evaluate the flow at the in-between
        time -- N rounds of g = bilinear flow at (p - t g) per output pixel and time -- before they warp.  The flows handed out
        and the estimate entry points are unchanged."""
        self._check(self._lib.nus_flow_set_project(self._h, check_project(rounds)))

    @property
    def project(self) -> int:
        return int(self._lib.nus_flow_project_rounds(self._h))

    def set_bidirectional(self, enabled: bool) -> None:
        """Both flows of every pair and the select warp behind the estimator (nus_flow_set_bidirectional; off by default):
        `interpolate_device_stream` and `interpolate_multi_device_stream` also estimate every pair B -> A on the same pyramids, and
        each output pixel is warped with the forward vector or the negated backward one, whichever makes its sample of A and its
        sample of B agree better.  The flows handed out are the forward ones, unchanged; the estimate entry points are not
        affected; `retime_device_stream` refuses the setting (ValueError) -- rate conversion with the select warp is
        `retime_select_device_stream`, which does not look at it."""
        if not isinstance(enabled, (bool, np.bool_)) and enabled not in (0, 1):
            raise ValueError(f"bidirectional must be a bool, got {enabled!r}")
        self._check(self._lib.nus_flow_set_bidirectional(self._h, 1 if enabled else 0))

    @property
    def bidirectional(self) -> bool:
        return self._lib.nus_flow_bidirectional(self._h) == 1

    @property
    def workspace_bytes(self) -> int:
        """Bytes of device workspace the handle holds now (nus_flow_workspace_bytes; grow-only)."""
        return int(self._lib.nus_flow_workspace_bytes(self._h))

    def _fill_workspace(self, byte: int, stream: int = 0) -> None:
        """TEST HOOK (nus_flow_fill_workspace; the process needs NUS_TEST_HOOKS=1): every byte of the handle's device workspace set
        to `byte` on `stream`, which is synchronised before this returns."""
        self._check(self._lib.nus_flow_fill_workspace(self._h, int(byte), stream or None))

    def set_scene_detect(self, enabled: bool, mad_threshold: int = C.SCENE_DEFAULT_MAD,
                         hist_permille: int = C.SCENE_DEFAULT_HIST_PERMILLE) -> None:
        """Scene-cut detection in front of `interpolate_multi_device_stream` (nus_flow_set_scene_detect; off by default): the
        in-between frames of a pair the detector flags are repeats of the nearer real frame."""
        from .scene import check_thresholds

        mad, hist = check_thresholds(mad_threshold, hist_permille)
        self._check(self._lib.nus_flow_set_scene_detect(self._h, 1 if enabled else 0, mad, hist))

    @property
    def mode(self) -> str:
        return "fast" if self._lib.nus_flow_mode(self._h) == 1 else "exact"

    def _check(self, status: int) -> None:
        if status != C.OK:
            raise RuntimeError(self._lib.nus_flow_last_error(self._h).decode("utf-8", "replace"))

    @staticmethod
    def _f32(a, shape=None):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if shape is not None and a.shape != shape:
            raise ValueError(f"expected shape {shape}, got {a.shape}")
        return a

    # ---- primitives (host arrays in / out) ----------------------------------------
    def rgba8_to_f32(self, img: np.ndarray) -> np.ndarray:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape[:2]
        out = np.empty((h, w, 4), np.float32)
        self._check(self._lib.nus_flow_rgba8_to_f32(self._h, img.ctypes.data, w, h, out.ctypes.data))
        return out

    def blur(self, img: np.ndarray) -> np.ndarray:
        img = self._f32(img)
        h, w = img.shape[:2]
        out = np.empty_like(img)
        self._check(self._lib.nus_flow_blur(self._h, img.ctypes.data, w, h, out.ctypes.data))
        return out

    def downsample(self, img: np.ndarray) -> np.ndarray:
        img = self._f32(img)
        h, w = img.shape[:2]
        out = np.empty(((h + 1) // 2, (w + 1) // 2, 4), np.float32)
        self._check(self._lib.nus_flow_downsample(self._h, img.ctypes.data, w, h, out.ctypes.data))
        return out

    def horn_schunck(self, i1: np.ndarray, i2: np.ndarray, flow_in=None, iterations: int = 1, lambda_=None) -> np.ndarray:
        i1, i2 = self._f32(i1), self._f32(i2, np.shape(i1))
        h, w = i1.shape[:2]
        fin = None if flow_in is None else self._f32(flow_in, (h, w, 2))
        out = np.empty((h, w, 2), np.float32)
        self._check(self._lib.nus_flow_horn_schunck(self._h, i1.ctypes.data, i2.ctypes.data,
                                                    None if fin is None else fin.ctypes.data, w, h,
                                                    self.lambda_ if lambda_ is None else float(lambda_),
                                                    int(iterations), out.ctypes.data))
        return out

    def warp_coefficients(self, i1: np.ndarray, i2: np.ndarray, flow=None) -> np.ndarray:
        """(h, w, 3) float32 (Ix, Iy, It') of two f32 RGBA images, frame 2's luminance sampled through `flow` ((h, w, 2); None: zero
        flow, It = L2 - L1): what a re-linearised level's Jacobi steps run on (nus_flow_warp_coefficients)."""
        i1, i2 = self._f32(i1), self._f32(i2, np.shape(i1))
        h, w = i1.shape[:2]
        fl = None if flow is None else self._f32(flow, (h, w, 2))
        out = np.empty((h, w, 3), np.float32)
        self._check(self._lib.nus_flow_warp_coefficients(self._h, i1.ctypes.data, i2.ctypes.data, None if fl is None else fl.ctypes.data,
                                                         w, h, out.ctypes.data))
        return out

    def horn_schunck_coef(self, coef: np.ndarray, flow_in=None, iterations: int = 1, lambda_=None) -> np.ndarray:
        """`iterations` Jacobi steps on (h, w, 3) coefficients (Ix, Iy, It), from `flow_in` (None: zero flow)."""
        coef = self._f32(coef)
        if coef.ndim != 3 or coef.shape[2] != 3:
            raise ValueError(f"expected (h, w, 3) coefficients, got {coef.shape}")
        h, w = coef.shape[:2]
        fin = None if flow_in is None else self._f32(flow_in, (h, w, 2))
        out = np.empty((h, w, 2), np.float32)
        self._check(self._lib.nus_flow_horn_schunck_coef(self._h, coef.ctypes.data, None if fin is None else fin.ctypes.data, w, h,
                                                         self.lambda_ if lambda_ is None else float(lambda_), int(iterations),
                                                         out.ctypes.data))
        return out

    def upsample(self, flow: np.ndarray, dw: int, dh: int, scale: float = 1.0) -> np.ndarray:
        flow = self._f32(flow)
        sh, sw = flow.shape[:2]
        out = np.empty((dh, dw, 2), np.float32)
        self._check(self._lib.nus_flow_upsample(self._h, flow.ctypes.data, sw, sh, out.ctypes.data, dw, dh, float(scale)))
        return out

    def median(self, flow: np.ndarray, size: int) -> np.ndarray:
        """The component-wise size x size median (3 or 5) of an (h, w, 2) flow, border replicated: the stage `set_median` adds
        behind every Jacobi run, on its own (nus_flow_median)."""
        flow = self._f32(flow)
        if flow.ndim != 3 or flow.shape[2] != 2:
            raise ValueError(f"expected an (h, w, 2) flow, got {flow.shape}")
        if isinstance(size, bool) or size not in (3, 5):
            raise ValueError(f"median size must be 3 or 5, got {size!r}")
        h, w = flow.shape[:2]
        out = np.empty((h, w, 2), np.float32)
        self._check(self._lib.nus_flow_median(self._h, flow.ctypes.data, w, h, int(size), out.ctypes.data))
        return out

    def project_flow(self, flow: np.ndarray, t: float, rounds: int) -> np.ndarray:
        """The vector every output pixel of the in-between frame at time t is warped with after `rounds` projection rounds of an
        (h, w, 2) flow: the stage `set_project` / `WgpuFrameInterpolator.set_flow_project` put in front of the warp, on its own
        (nus_flow_project)."""
        flow = self._f32(flow)
        if flow.ndim != 3 or flow.shape[2] != 2:
            raise ValueError(f"expected an (h, w, 2) flow, got {flow.shape}")
        rounds = check_project(rounds)
        t = float(t)
        if t != t:
            raise ValueError("project_flow: t is NaN")
        h, w = flow.shape[:2]
        out = np.empty((h, w, 2), np.float32)
        self._check(self._lib.nus_flow_project(self._h, flow.ctypes.data, w, h, t, rounds, out.ctypes.data))
        return out

    # ---- full estimator ------------------------------------------------------------
    def estimate(self, frame_a, frame_b, width: int, height: int) -> np.ndarray:
        """RGBA8 frames (bytes or arrays) -> (h, w, 2) float32 flow, pixel delta A -> B."""
        a = np.frombuffer(frame_a, np.uint8) if isinstance(frame_a, (bytes, bytearray, memoryview)) else np.ascontiguousarray(frame_a, np.uint8)
        b = np.frombuffer(frame_b, np.uint8) if isinstance(frame_b, (bytes, bytearray, memoryview)) else np.ascontiguousarray(frame_b, np.uint8)
        n = width * height * 4
        if a.size != n or b.size != n:
            raise ValueError(f"Expected {n} bytes per frame for {width}x{height}x4 RGBA, got frame_a: {a.size} bytes, frame_b: {b.size} bytes")
        out = np.empty((height, width, 2), np.float32)
        self._check(self._lib.nus_flow_estimate(self._h, a.ctypes.data, b.ctypes.data, width, height, self.levels,
                                                self.coarse_iterations, self.refine_iterations, self.lambda_,
                                                out.ctypes.data))
        return out

    def estimate_device(self, d_a: int, d_b: int, width: int, height: int, d_flow_out: int, stream: int = 0) -> None:
        self._check(self._lib.nus_flow_estimate_device(self._h, d_a, d_b, width, height, self.levels,
                                                       self.coarse_iterations, self.refine_iterations, self.lambda_,
                                                       d_flow_out, stream or None))

    def estimate_device_stream(self, d_frames: int, n_frames: int, width: int, height: int, d_flows: int,
                               stream: int = 0) -> None:
        """`n_frames` consecutive RGBA8 frames on the device -> `n_frames - 1` flows (k -> k+1) at `d_flows`;
        same result as one `estimate_device` per pair, each frame's pyramid built once."""
        self._check(self._lib.nus_flow_estimate_device_stream(self._h, d_frames, n_frames, width, height, self.levels,
                                                              self.coarse_iterations, self.refine_iterations,
                                                              self.lambda_, d_flows, stream or None))

    def interpolate_device_stream(self, d_frames: int, n_frames: int, width: int, height: int, time_t: float, d_mid: int,
                                  d_flows: int = 0, stream: int = 0, flow_format: str = "f32") -> None:
        """The reference's intended interpolate() as one pipeline (wgpu_interpolator.rs:881-935: pyramid -> coarse flow -> warp):
        `n_frames` consecutive RGBA8 frames on the device -> the `n_frames - 1` in-between frames at `time_t` at `d_mid`, warped +
        blended with each pair's flow (FMA-mode warp), and the flows themselves at `d_flows` if that is not 0
        (nus_flow_interpolate_device_stream).  flow_format "f16": the flows between estimator and warp (and at `d_flows`) as
        Rg16Float, the reference's live layout -- the f32 flow rounded to nearest even, read as such by the warp."""
        fmt = {"f32": 0, "f16": 1}.get(flow_format)
        if fmt is None:
            raise ValueError("flow_format must be 'f32' or 'f16'")
        self._check(self._lib.nus_flow_interpolate_device_stream(self._h, d_frames, n_frames, width, height, self.levels,
                                                                 self.coarse_iterations, self.refine_iterations, self.lambda_,
                                                                 float(time_t), fmt, d_flows or None, d_mid, stream or None))

    def interpolate_multi_device_stream(self, d_frames: int, n_frames: int, width: int, height: int, times, d_mid: int,
                                        d_flows: int = 0, mid_pair_stride: int = 0, stream: int = 0, flow_format: str = "f32") -> None:
        """interpolate_device_stream at several times per pair (nus_flow_interpolate_multi_device_stream): each pair's flow is
        estimated once and all its frames are warped from it; pair k's frame j at d_mid + k * mid_pair_stride + j * w*h*4
        (0: tightly packed)."""
        fmt = {"f32": 0, "f16": 1}.get(flow_format)
        if fmt is None:
            raise ValueError("flow_format must be 'f32' or 'f16'")
        ts = (ctypes.c_float * len(times))(*[float(t) for t in times])
        self._check(self._lib.nus_flow_interpolate_multi_device_stream(self._h, d_frames, n_frames, width, height, self.levels,
                                                                       self.coarse_iterations, self.refine_iterations, self.lambda_,
                                                                       ts, len(times), fmt, d_flows or None, d_mid, mid_pair_stride,
                                                                       stream or None))

    def retime_device_stream(self, d_frames: int, n_frames: int, width: int, height: int, num: int, den: int, d_out: int,
                             d_flows: int = 0, out_frame_stride: int = 0, stream: int = 0, flow_format: str = "f32") -> None:
        """The stream converted by num / den (nus_flow_retime_device_stream; retime.py has the schedule): each pair's flow is
        estimated once, then the retime warp in FMA mode writes output j at d_out + j * out_frame_stride (0: tightly packed), real
        frames included; the flows at `d_flows` if that is not 0.  Warps, median, projection rounds and scene detection as the
        handle is set."""
        fmt = {"f32": 0, "f16": 1}.get(flow_format)
        if fmt is None:
            raise ValueError("flow_format must be 'f32' or 'f16'")
        st = self._lib.nus_flow_retime_device_stream(self._h, d_frames or None, int(n_frames), int(width), int(height), self.levels,
                                                     self.coarse_iterations, self.refine_iterations, self.lambda_, int(num), int(den), fmt,
                                                     d_flows or None, d_out or None, int(out_frame_stride), stream or None)
        if st == C.ERR_INVALID_ARGUMENT and self.bidirectional:  # refused before any GPU work: the C text
            raise ValueError(self._lib.nus_flow_last_error(self._h).decode("utf-8", "replace"))
        self._check(st)

    def estimate_both_device_stream(self, d_frames: int, n_frames: int, width: int, height: int, d_flows_fwd: int, d_flows_bwd: int,
                                    stream: int = 0) -> None:
        """Both flows of every pair (nus_flow_estimate_both_device_stream), f32: `d_flows_fwd` receives the bytes of
        `estimate_device_stream`, `d_flows_bwd` pair k's flow frame k+1 -> frame k on frame k+1's grid -- the backward solve of
        `set_bidirectional`, handed out.  Does not look at that setting.  Argument errors raise ValueError before any GPU work."""
        st = self._lib.nus_flow_estimate_both_device_stream(self._h, d_frames or None, int(n_frames), int(width), int(height), self.levels,
                                                            self.coarse_iterations, self.refine_iterations, self.lambda_,
                                                            d_flows_fwd or None, d_flows_bwd or None, stream or None)
        if st == C.ERR_INVALID_ARGUMENT:
            raise ValueError(self._lib.nus_flow_last_error(self._h).decode("utf-8", "replace"))
        self._check(st)

    def retime_select_device_stream(self, d_frames: int, n_frames: int, width: int, height: int, num: int, den: int, d_out: int,
                                    d_flows_fwd: int = 0, d_flows_bwd: int = 0, out_frame_stride: int = 0, stream: int = 0,
                                    flow_format: str = "f32") -> None:
        """`retime_device_stream` with both flows of every pair and the select warp (nus_flow_retime_select_device_stream): the
        bytes of `estimate_both_device_stream` followed by `WgpuFrameInterpolator.retime_select_device` in FMA mode.  The flows at
        `d_flows_fwd` / `d_flows_bwd` where those are not 0.  Does not look at `set_bidirectional`.  Argument errors raise
        ValueError before any GPU work."""
        fmt = {"f32": 0, "f16": 1}.get(flow_format)
        if fmt is None:
            raise ValueError("flow_format must be 'f32' or 'f16'")
        st = self._lib.nus_flow_retime_select_device_stream(self._h, d_frames or None, int(n_frames), int(width), int(height), self.levels,
                                                            self.coarse_iterations, self.refine_iterations, self.lambda_, int(num),
                                                            int(den), fmt, d_flows_fwd or None, d_flows_bwd or None, d_out or None,
                                                            int(out_frame_stride), stream or None)
        if st == C.ERR_INVALID_ARGUMENT:
            raise ValueError(self._lib.nus_flow_last_error(self._h).decode("utf-8", "replace"))
        self._check(st)
