"""Python mirror of the reference's `WgpuFrameInterpolator` pyclass
(nu_scaler_core/src/wgpu_interpolator.rs:130-498), bound to the HIP C ABI."""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import numpy as np

from . import _capi as C
from .upscaler import _as_buffer, _out_buffer

_PRESETS = {  # wgpu_interpolator.rs:117-125
    "8x8": C.WG_SQUARE_8X8, "square8x8": C.WG_SQUARE_8X8,
    "16x16": C.WG_SQUARE_16X16, "square16x16": C.WG_SQUARE_16X16,
    "32x8": C.WG_WIDE_32X8, "wide32x8": C.WG_WIDE_32X8, "wide": C.WG_WIDE_32X8,
    "8x32": C.WG_TALL_8X32, "tall8x32": C.WG_TALL_8X32, "tall": C.WG_TALL_8X32,
}


def frame_times(multiplier: int) -> list[float]:
    """The in-between times of a frame-rate multiplier M (the GUI's "Frame Generation" slider: 2x, 3x, 4x ...): k / M for
    k = 1 .. M - 1, each rounded to float32 as the kernels take it.  M from 2 to INTERP_MAX_TIMES + 1 (8)."""
    if isinstance(multiplier, bool) or not isinstance(multiplier, (int, np.integer)):
        raise ValueError(f"multiplier must be an integer from 2 to {C.INTERP_MAX_TIMES + 1}, got {multiplier!r}")
    m = int(multiplier)
    if not 2 <= m <= C.INTERP_MAX_TIMES + 1:
        raise ValueError(f"multiplier must be from 2 to {C.INTERP_MAX_TIMES + 1}, got {m}")
    return [float(np.float32(k / m)) for k in range(1, m)]


def _time_array(times=None, multiplier=None) -> "ctypes.Array":
    """The float32 time set of a multi-time call: exactly one of `times` and `multiplier`, checked here (ValueError) before any
    GPU work, with the library's rules: 1 .. INTERP_MAX_TIMES times, each in [0, 1]."""
    if (times is None) == (multiplier is None):
        raise ValueError("give exactly one of times and multiplier")
    ts = frame_times(multiplier) if multiplier is not None else [float(np.float32(t)) for t in times]
    if not 1 <= len(ts) <= C.INTERP_MAX_TIMES:
        raise ValueError(f"between 1 and {C.INTERP_MAX_TIMES} times per call, got {len(ts)}")
    for t in ts:
        if math.isnan(t) or not 0.0 <= t <= 1.0:
            raise ValueError(f"every time must be in [0, 1], got {t}")
    return (ctypes.c_float * len(ts))(*ts)


class WgpuFrameInterpolator:
    """`WgpuFrameInterpolator(workgroup_preset_str=None)` (wgpu_interpolator.rs:172-174).
    Unknown / missing presets default to Wide32x8 as in the reference; the preset is
    recorded only -- the HIP kernels use their own wave64 launch shape (and, unlike the
    reference's dispatch at :372-374, always cover the whole frame)."""

    def __init__(self, workgroup_preset_str: Optional[str] = None, *, device: int = 0):
        self._lib = C.lib()
        preset = _PRESETS.get(str(workgroup_preset_str).lower(), C.WG_WIDE_32X8) if workgroup_preset_str else C.WG_WIDE_32X8
        self._h = self._lib.nus_interp_create(preset)
        if not self._h:
            raise RuntimeError(C.last_error())
        if self._lib.nus_interp_set_device(self._h, int(device)) != C.OK:
            raise RuntimeError(self._err())
        self._device, self._format = int(device), C.FORMAT_RGBA8

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.nus_interp_destroy(h)

    def _err(self) -> str:
        return self._lib.nus_interp_last_error(self._h).decode("utf-8", "replace")

    def _raise(self, status: int) -> None:
        if status == C.OK:
            return
        msg = self._err()
        if status == C.ERR_SIZE_MISMATCH:  # PyValueError at wgpu_interpolator.rs:233-238
            raise ValueError(msg)
        raise RuntimeError(msg)

    def interpolate_py(self, frame_a_bytes, frame_b_bytes, width: int, height: int, *, time_t: float = 0.5,
                       flow=None) -> bytes:
        """wgpu_interpolator.rs:215-225.  `flow` (optional, not in the reference's
        signature): (h, w, 2) float32 buffer of pixel deltas A->B; None = zero flow,
        which is what the reference always uses."""
        a_addr, a_len, ka = _as_buffer(frame_a_bytes)
        b_addr, b_len, kb = _as_buffer(frame_b_bytes)
        f_addr, kf = None, None
        expected = int(width) * int(height) * 4
        if flow is not None:
            f_addr, f_len, kf = _as_buffer(flow)
            if f_len != expected * 2:
                raise ValueError(f"Expected {expected * 2} bytes of flow for {width}x{height}x2 f32, got {f_len}")
        out, oarr, oaddr = _out_buffer(expected)
        st = self._lib.nus_interp_interpolate(self._h, a_addr, a_len, b_addr, b_len, f_addr, width, height,
                                              float(time_t), oaddr, expected)
        del oarr, ka, kb, kf
        self._raise(st)
        return out

    def interpolate_multi_py(self, frame_a_bytes, frame_b_bytes, width: int, height: int, *, times: Optional[Sequence[float]] = None,
                             multiplier: Optional[int] = None, flow=None, scene_detect=False) -> list[bytes]:
        """The in-between frames of one pair at several times from one launch (nus_interp_interpolate_multi): at `times`, or at
        frame_times(multiplier).  Each frame is what interpolate_py returns at that time.  Argument errors raise ValueError
        before any GPU work.  `scene_detect` (False; True for the default thresholds, or a `SceneDetector`): if the detector
        flags the pair as a scene cut, every frame is a repeat of the nearer real frame -- the zero-flow launch at t = 0 (times
        below one half) or t = 1, which is the copy nus_scene_apply_cuts_device defines."""
        ts = _time_array(times, multiplier)
        n = len(ts)
        if scene_detect:
            from .scene import SceneDetector

            det = scene_detect if isinstance(scene_detect, SceneDetector) else SceneDetector(device=self._device)
            if det.detect(frame_a_bytes, frame_b_bytes, width, height, fmt=self._format)[0]:
                ts, flow = (ctypes.c_float * n)(*[0.0 if t < 0.5 else 1.0 for t in ts]), None
        a_addr, a_len, ka = _as_buffer(frame_a_bytes)
        b_addr, b_len, kb = _as_buffer(frame_b_bytes)
        f_addr, kf = None, None
        expected = int(width) * int(height) * 4
        if flow is not None:
            f_addr, f_len, kf = _as_buffer(flow)
            if f_len != expected * 2:
                raise ValueError(f"Expected {expected * 2} bytes of flow for {width}x{height}x2 f32, got {f_len}")
        out, oarr, oaddr = _out_buffer(expected * n)
        st = self._lib.nus_interp_interpolate_multi(self._h, a_addr, a_len, b_addr, b_len, f_addr, width, height, ts, n, oaddr,
                                                    expected * n)
        del oarr, ka, kb, kf
        self._raise(st)
        mv = memoryview(out)
        return [bytes(mv[k * expected:(k + 1) * expected]) for k in range(n)]

    def interpolate_multi_device(self, d_a: int, a_stride: int, d_b: int, b_stride: int, d_flow: int, width: int, height: int,
                                 times: Sequence[float], d_out: int, out_pair_stride: int = 0, n_pairs: int = 1,
                                 stream: int = 0) -> None:
        """nus_interp_interpolate_multi_device: frame (i, k) at d_out + i * out_pair_stride + k * w*h*4 (0: tightly packed)."""
        ts = (ctypes.c_float * len(times))(*[float(t) for t in times])
        self._raise(self._lib.nus_interp_interpolate_multi_device(self._h, d_a, a_stride, d_b, b_stride, d_flow or None, width,
                                                                  height, ts, len(times), d_out, out_pair_stride, n_pairs,
                                                                  stream or None))

    def _flow_buffer(self, flow, name: str, expected: int):
        if flow is None:
            raise ValueError(f"{name} is required: the select warp takes both flows")
        addr, length, keep = _as_buffer(flow)
        if length != expected * 2:
            raise ValueError(f"Expected {expected * 2} bytes of {name} for 2 f32 per pixel, got {length}")
        return addr, keep

    def interpolate_select_multi_py(self, frame_a_bytes, frame_b_bytes, width: int, height: int, flow_fwd, flow_bwd, *,
                                    times: Optional[Sequence[float]] = None, multiplier: Optional[int] = None) -> list[bytes]:
        """The select warp (nus_interp_interpolate_select): `flow_fwd` is the flow A -> B on A's grid, `flow_bwd` the flow B -> A
        on B's grid, both (h, w, 2) float32.  Each output pixel is warped with the forward vector or with the negated backward
        one -- both evaluated at the in-between time with the handle's projection rounds -- whichever makes its sample of A and
        its sample of B agree better over the three colour bytes; a tie goes forward.  The frames at `times`, or at
        frame_times(multiplier).  Argument errors raise ValueError before any GPU work."""
        ts = _time_array(times, multiplier)
        n = len(ts)
        a_addr, a_len, ka = _as_buffer(frame_a_bytes)
        b_addr, b_len, kb = _as_buffer(frame_b_bytes)
        expected = int(width) * int(height) * 4
        f_addr, kf = self._flow_buffer(flow_fwd, "flow_fwd", expected)
        r_addr, kr = self._flow_buffer(flow_bwd, "flow_bwd", expected)
        out, oarr, oaddr = _out_buffer(expected * n)
        st = self._lib.nus_interp_interpolate_select(self._h, a_addr, a_len, b_addr, b_len, f_addr, r_addr, width, height, ts, n,
                                                     oaddr, expected * n)
        del oarr, ka, kb, kf, kr
        self._raise(st)
        mv = memoryview(out)
        return [bytes(mv[k * expected:(k + 1) * expected]) for k in range(n)]

    def interpolate_select_py(self, frame_a_bytes, frame_b_bytes, width: int, height: int, flow_fwd, flow_bwd, *,
                              time_t: float = 0.5) -> bytes:
        """One frame of the select warp at `time_t` in [0, 1]: see interpolate_select_multi_py."""
        return self.interpolate_select_multi_py(frame_a_bytes, frame_b_bytes, width, height, flow_fwd, flow_bwd, times=[time_t])[0]

    def interpolate_select_device(self, d_a: int, a_stride: int, d_b: int, b_stride: int, d_flow_fwd: int, d_flow_bwd: int,
                                  width: int, height: int, times: Sequence[float], d_out: int, out_pair_stride: int = 0,
                                  n_pairs: int = 1, stream: int = 0) -> None:
        """nus_interp_interpolate_select_device: as interpolate_multi_device with both flows of every pair, in the handle's
        flow format.  Argument errors raise ValueError before any GPU work."""
        ts = (ctypes.c_float * len(times))(*[float(t) for t in times])
        st = self._lib.nus_interp_interpolate_select_device(self._h, d_a, a_stride, d_b, b_stride, d_flow_fwd or None,
                                                            d_flow_bwd or None, width, height, ts, len(times), d_out,
                                                            out_pair_stride, n_pairs, stream or None)
        if st == C.ERR_INVALID_ARGUMENT:
            raise ValueError(self._err())
        self._raise(st)

    def retime_device(self, d_frames: int, frame_stride: int, n_frames: int, d_flows: int, width: int, height: int, num: int,
                      den: int, d_out: int, out_frame_stride: int = 0, stream: int = 0) -> None:
        """nus_interp_retime_device: the device-resident stream of `n_frames` frames converted by num / den (retime.py has the
        schedule); pair k's flow at d_flows + k * flow bytes (0: zero flow); output j at d_out + j * out_frame_stride (0: tightly
        packed).  Argument errors raise ValueError before any GPU work."""
        st = self._lib.nus_interp_retime_device(self._h, d_frames or None, int(frame_stride), int(n_frames), d_flows or None,
                                                int(width), int(height), int(num), int(den), d_out or None, int(out_frame_stride),
                                                stream or None)
        if st == C.ERR_INVALID_ARGUMENT:
            raise ValueError(self._err())
        self._raise(st)

    def retime_select_device(self, d_frames: int, frame_stride: int, n_frames: int, d_flows_fwd: int, d_flows_bwd: int, width: int,
                             height: int, num: int, den: int, d_out: int, out_frame_stride: int = 0, stream: int = 0) -> None:
        """nus_interp_retime_select_device: `retime_device` with both flows of every pair and the select warp -- pair k's forward
        plane on frame k's grid, its backward plane on frame k + 1's, both required, in the handle's flow format.  Argument errors
        raise ValueError before any GPU work."""
        st = self._lib.nus_interp_retime_select_device(self._h, d_frames or None, int(frame_stride), int(n_frames), d_flows_fwd or None,
                                                       d_flows_bwd or None, int(width), int(height), int(num), int(den), d_out or None,
                                                       int(out_frame_stride), stream or None)
        if st == C.ERR_INVALID_ARGUMENT:
            raise ValueError(self._err())
        self._raise(st)

    # -- trait FrameInterpolator (nu_scaler_core/src/interpolation/mod.rs:29-44; dead code in the reference, same shape here)
    def initialize(self, width: int, height: int) -> None:
        self._raise(self._lib.nus_interp_initialize(self._h, int(width), int(height)))

    def interpolate(self, frame1, frame2, t: float) -> bytes:
        """Frames of the initialize() size, zero flow; RuntimeError("Interpolator not initialized") before it."""
        a_addr, a_len, ka = _as_buffer(frame1)
        b_addr, b_len, kb = _as_buffer(frame2)
        out, oarr, oaddr = _out_buffer(a_len)
        st = self._lib.nus_interp_interpolate_frames(self._h, a_addr, a_len, b_addr, b_len, float(t), oaddr, a_len)
        del oarr, ka, kb
        self._raise(st)
        return out

    @property
    def name(self) -> str:
        return self._lib.nus_interp_name(self._h).decode()

    _QUALITY = {"high": 0, "medium": 1, "low": 2}

    def set_quality(self, quality) -> None:
        q = self._QUALITY.get(str(quality).lower(), quality)
        self._raise(self._lib.nus_interp_set_quality(self._h, int(q)))

    @property
    def quality(self) -> str:
        return ("high", "medium", "low")[self._lib.nus_interp_quality(self._h)]

    def interpolate_device(self, d_a: int, a_stride: int, d_b: int, b_stride: int, d_flow: int, width: int,
                           height: int, time_t: float, d_out: int, n_pairs: int = 1, stream: int = 0) -> None:
        self._raise(self._lib.nus_interp_interpolate_device(self._h, d_a, a_stride, d_b, b_stride, d_flow or None,
                                                            width, height, float(time_t), d_out, n_pairs, stream or None))

    def set_input_format(self, fmt: str) -> None:
        """"rgba" (default) or "bgra" for both input frames; the new frame is RGBA."""
        f = {"rgba": C.FORMAT_RGBA8, "bgra": C.FORMAT_BGRA8, "rgbx": C.FORMAT_RGBX8, "bgrx": C.FORMAT_BGRX8}.get(str(fmt).lower())
        if f is None:
            raise ValueError("input format must be 'rgba', 'bgra', 'rgbx' or 'bgrx'")
        self._raise(self._lib.nus_interp_set_input_format(self._h, f))
        self._format = f

    def set_mode(self, mode: str) -> None:
        """Arithmetic of the dense-flow warp: "exact" (default; the CPU's roundings, bit-exact against the oracle) or "fma"
        (fused lerps, within 1 LSB).  The zero-flow blend is exact either way."""
        m = {"exact": 0, "fma": 1}.get(str(mode).lower())
        if m is None:
            raise ValueError("mode must be 'exact' or 'fma'")
        self._raise(self._lib.nus_interp_set_mode(self._h, m))

    @property
    def mode(self) -> str:
        return "fma" if self._lib.nus_interp_mode(self._h) == 1 else "exact"

    def set_flow_project(self, rounds: int) -> None:
        """Projection rounds of the dense-flow warp (nus_interp_set_flow_project; 0, the default, is off; at most
        FLOW_MAX_PROJECT): the flow lives on frame A's grid, so each output pixel first looks its vector up where its content came
        from -- N rounds of g = bilinear flow at (p - t g) -- and is then warped with g.  Removes the wrong ring around moving
        objects; 2 never loses on the float64 witness, 3 gains most.  Applies to every call given a flow."""
        from .flow import check_project

        self._raise(self._lib.nus_interp_set_flow_project(self._h, check_project(rounds)))

    @property
    def flow_project(self) -> int:
        return int(self._lib.nus_interp_flow_project(self._h))

    def set_flow_format(self, fmt: str) -> None:
        """Element type of the device flow field `interpolate_device` reads: "f32" (default, 2 x f32 per pixel) or
        "f16" (2 x half per pixel: the Rg16Float texture of wgpu_interpolator.rs:276, half the bytes)."""
        f = {"f32": 0, "f16": 1}.get(str(fmt).lower())
        if f is None:
            raise ValueError("flow format must be 'f32' or 'f16'")
        self._raise(self._lib.nus_interp_set_flow_format(self._h, f))

    def get_last_gpu_duration_ms(self) -> Optional[float]:
        """wgpu_interpolator.rs:494-497: None until an interpolation has run."""
        ms = ctypes.c_double()
        return ms.value if self._lib.nus_interp_last_gpu_ms(self._h, ctypes.byref(ms)) == C.OK else None
