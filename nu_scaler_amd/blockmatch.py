"""Block-matching motion estimation on the HIP device: the reference's `BlockMatchingInterpolator`
(nu_scaler_core/src/interpolation/mod.rs:513-911) as `BlockMatcher`, bound to `nus_bm_*` of include/nuscaler_hip.h (the
definitions are written there), and its pyclass `PyFrameInterpolator` (:959-1049).  No torch type crosses into this module: the
device entry point takes integer device addresses, as `WgpuFrameInterpolator.interpolate_device` does."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _capi as C
from .interpolator import WgpuFrameInterpolator, _time_array
from .upscaler import _as_buffer, _out_buffer

_QUALITY = {"high": C.INTERP_QUALITY_HIGH, "medium": C.INTERP_QUALITY_MEDIUM, "low": C.INTERP_QUALITY_LOW}
_QUALITY_NAMES = ("high", "medium", "low")
PRESETS = {"high": (8, 24), "medium": (16, 16), "low": (32, 8)}  # (block_size, search_radius), interpolation/mod.rs:531-542
_ORDER = {"scan": C.BM_TIES_SCAN, "center": C.BM_TIES_CENTER}
_FLOW = {"f32": C.FLOW_F32, "f16": C.FLOW_F16}
_MODE = {"exact": C.INTERP_MODE_EXACT, "fma": C.INTERP_MODE_FMA}


def block_grid(w: int, h: int, block_size: int) -> tuple[int, int]:
    """(blocks_x, blocks_y) = (ceil(w / bs), ceil(h / bs)): partial blocks at the right and bottom edge count."""
    bs = int(block_size)
    return -(-int(w) // bs), -(-int(h) // bs)


class BlockMatcher:
    """Full-search block matching of RGBA8 frame pairs.  `quality` picks a preset ("high" 8 / 24, "medium" 16 / 16, "low" 32 / 8);
    `block_size` (8, 16, 32) and `search_radius` (1 .. 24) override it.  `tie_order`: "center" (default: the smallest
    displacement among equal SADs) or "scan" (the reference's first minimum in dy-major order).  `refine`: the confidence pass.
    `bidirectional`: the forward-backward check with `tolerance` (see set_bidirectional) in place of that pass."""

    def __init__(self, quality: str = "medium", *, block_size: Optional[int] = None, search_radius: Optional[int] = None,
                 tie_order: str = "center", refine: bool = True, bidirectional: bool = False,
                 tolerance: int = C.BM_BIDIR_DEFAULT_TOLERANCE, device: int = 0):
        self._lib = C.lib()
        self._h = self._lib.nus_bm_create()
        if not self._h:
            raise RuntimeError(C.last_error())
        self._check(self._lib.nus_bm_set_device(self._h, int(device)))
        bs, radius = PRESETS.get(str(quality).lower(), PRESETS["medium"])
        self.set_params(bs if block_size is None else block_size, radius if search_radius is None else search_radius)
        self.set_tie_order(tie_order)
        self.set_refine(refine)
        self.set_bidirectional(bidirectional, tolerance)
        self.scene_detect, self._scene_thresholds = False, (C.SCENE_DEFAULT_MAD, C.SCENE_DEFAULT_HIST_PERMILLE)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.nus_bm_destroy(h)

    def _check(self, status: int) -> None:
        if status == C.OK:
            return
        msg = self._lib.nus_bm_last_error(self._h).decode("utf-8", "replace")
        raise ValueError(msg) if status in (C.ERR_INVALID_ARGUMENT, C.ERR_SIZE_MISMATCH) else RuntimeError(msg)

    def set_params(self, block_size: int, search_radius: int) -> None:
        self._check(self._lib.nus_bm_set_params(self._h, int(block_size), int(search_radius)))
        self.block_size, self.search_radius = int(block_size), int(search_radius)

    def set_quality(self, quality: str) -> None:
        q = str(quality).lower()
        if q not in _QUALITY:
            raise ValueError("Invalid quality setting")
        self._check(self._lib.nus_bm_set_quality(self._h, _QUALITY[q]))
        self.block_size, self.search_radius = PRESETS[q]

    def set_tie_order(self, order: str) -> None:
        o = _ORDER.get(str(order).lower())
        if o is None:
            raise ValueError("tie order must be 'scan' or 'center'")
        self._check(self._lib.nus_bm_set_tie_order(self._h, o))
        self.tie_order = str(order).lower()

    def set_refine(self, enabled: bool) -> None:
        self._check(self._lib.nus_bm_set_refine(self._h, 1 if enabled else 0))
        self.refine = bool(enabled)

    def set_bidirectional(self, enabled: bool, tolerance: int = C.BM_BIDIR_DEFAULT_TOLERANCE) -> None:
        """Forward-backward check (nus_bm_set_bidirectional; off by default): every pair is searched both ways, a block whose
        two vectors do not answer each other within `tolerance` (0 .. 96, L1) takes the backward vector or the median of its
        neighbours, and the confidence pass is not run.  The search runs twice and both workspace sizes grow while it is on."""
        self._check(self._lib.nus_bm_set_bidirectional(self._h, 1 if enabled else 0, int(tolerance)))
        self.bidirectional, self.tolerance = bool(enabled), int(tolerance)

    def set_scene_detect(self, enabled: bool, mad_threshold: int = C.SCENE_DEFAULT_MAD,
                         hist_permille: int = C.SCENE_DEFAULT_HIST_PERMILLE) -> None:
        """Scene-cut detection in front of `interpolate` (nus_bm_set_scene_detect; off by default): the frames of a pair the
        detector flags are repeats of the nearer real frame."""
        from .scene import check_thresholds

        mad, hist = check_thresholds(mad_threshold, hist_permille)
        self._check(self._lib.nus_bm_set_scene_detect(self._h, 1 if enabled else 0, mad, hist))
        self.scene_detect, self._scene_thresholds = bool(enabled), (mad, hist)

    def block_grid(self, w: int, h: int) -> tuple[int, int]:
        return block_grid(w, h, self.block_size)

    def workspace_size(self, w: int, h: int, n_pairs: int = 1) -> int:
        """Bytes of device workspace `estimate_device` needs (nus_bm_workspace_size); ValueError for an invalid shape."""
        n = int(self._lib.nus_bm_workspace_size(self._h, int(w), int(h), int(n_pairs)))
        if n == 0:
            raise ValueError(self._lib.nus_bm_last_error(self._h).decode("utf-8", "replace"))
        return n

    def estimate_device(self, d_a: int, a_stride: int, d_b: int, b_stride: int, w: int, h: int, n_pairs: int, d_workspace: int,
                        workspace_bytes: int, d_vectors: int, d_sad: int = 0, d_flags: int = 0, d_flow: int = 0,
                        flow_format: str = "f32", stream: int = 0) -> None:
        """Enqueue the search of `n_pairs` pairs on `stream` (nus_bm_estimate_device): per block 2 x int16 at d_vectors, u32 at
        d_sad and u8 at d_flags (0: not wanted); the dense flow at d_flow (0: not wanted) as 2 x f32 or 2 x f16 per pixel."""
        fmt = _FLOW.get(str(flow_format).lower())
        if fmt is None:
            raise ValueError("flow format must be 'f32' or 'f16'")
        self._check(self._lib.nus_bm_estimate_device(self._h, d_a or None, int(a_stride), d_b or None, int(b_stride), int(w), int(h),
                                                     int(n_pairs), d_workspace or None, int(workspace_bytes), d_vectors or None,
                                                     d_sad or None, d_flags or None, d_flow or None, fmt, stream or None))

    def warp_device(self, d_a: int, a_stride: int, d_b: int, b_stride: int, w: int, h: int, n_pairs: int, d_vectors: int, d_out: int,
                    *, times: Optional[Sequence[float]] = None, multiplier: Optional[int] = None, mode: str = "exact",
                    out_pair_stride: int = 0, stream: int = 0) -> None:
        """Enqueue the warp + blend of `n_pairs` pairs straight from their block vectors (nus_bm_warp_device): `d_vectors` as
        `estimate_device` writes them at this block size; frame (i, k) at d_out + i * out_pair_stride + k * w*h*4 (0: tightly
        packed), at `times` or at frame_times(multiplier)."""
        m = _MODE.get(str(mode).lower())
        if m is None:
            raise ValueError("mode must be 'exact' or 'fma'")
        ts = _time_array(times, multiplier)
        self._check(self._lib.nus_bm_warp_device(self._h, d_a or None, int(a_stride), d_b or None, int(b_stride), int(w), int(h),
                                                 int(n_pairs), d_vectors or None, ts, len(ts), m, d_out or None, int(out_pair_stride),
                                                 stream or None))

    def stream_workspace_size(self, w: int, h: int, n_frames: int) -> int:
        """Bytes of device workspace `interpolate_stream_device` needs at the current settings (nus_bm_stream_workspace_size);
        ValueError for an invalid shape."""
        n = int(self._lib.nus_bm_stream_workspace_size(self._h, int(w), int(h), int(n_frames)))
        if n == 0:
            raise ValueError(self._lib.nus_bm_last_error(self._h).decode("utf-8", "replace"))
        return n

    def interpolate_stream_device(self, d_frames: int, frame_stride: int, n_frames: int, w: int, h: int, d_workspace: int,
                                  workspace_bytes: int, d_mid: int, *, times: Optional[Sequence[float]] = None,
                                  multiplier: Optional[int] = None, mode: str = "exact", d_vectors: int = 0,
                                  mid_pair_stride: int = 0, stream: int = 0) -> None:
        """Enqueue block-matched frame generation over `n_frames` device frames `frame_stride` bytes apart
        (nus_bm_interpolate_multi_device_stream): pair k = (frame k, frame k + 1), its frames at d_mid + k * mid_pair_stride +
        j * w*h*4; the pairs' vectors at d_vectors (0: not wanted).  Scene detection as set_scene_detect left it."""
        m = _MODE.get(str(mode).lower())
        if m is None:
            raise ValueError("mode must be 'exact' or 'fma'")
        ts = _time_array(times, multiplier)
        self._check(self._lib.nus_bm_interpolate_multi_device_stream(self._h, d_frames or None, int(frame_stride), int(n_frames), int(w),
                                                                     int(h), ts, len(ts), m, d_workspace or None, int(workspace_bytes),
                                                                     d_vectors or None, d_mid or None, int(mid_pair_stride),
                                                                     stream or None))

    def retime_stream_device(self, d_frames: int, frame_stride: int, n_frames: int, w: int, h: int, num: int, den: int,
                             d_workspace: int, workspace_bytes: int, d_out: int, *, mode: str = "exact", d_vectors: int = 0,
                             out_frame_stride: int = 0, stream: int = 0) -> None:
        """Enqueue the block-matched conversion of the stream by num / den (nus_bm_retime_device_stream; retime.py has the
        schedule): output j at d_out + j * out_frame_stride (0: tightly packed), real frames included; the workspace is
        stream_workspace_size's.  Scene detection as set_scene_detect left it."""
        m = _MODE.get(str(mode).lower())
        if m is None:
            raise ValueError("mode must be 'exact' or 'fma'")
        self._check(self._lib.nus_bm_retime_device_stream(self._h, d_frames or None, int(frame_stride), int(n_frames), int(w), int(h),
                                                          int(num), int(den), m, d_workspace or None, int(workspace_bytes),
                                                          d_vectors or None, d_out or None, int(out_frame_stride), stream or None))

    def estimate(self, frame_a, frame_b, w: int, h: int):
        """Host frames (bytes or uint8 arrays) -> (vectors int16 (blocks_y, blocks_x, 2) as (dx, dy), sad uint32 (blocks_y,
        blocks_x), flags uint8 (blocks_y, blocks_x))."""
        a_addr, a_len, ka = _as_buffer(frame_a)
        b_addr, b_len, kb = _as_buffer(frame_b)
        bx, by = self.block_grid(w, h) if int(w) > 0 and int(h) > 0 else (1, 1)
        vec = np.zeros((by, bx, 2), np.int16)
        sad = np.zeros((by, bx), np.uint32)
        flags = np.zeros((by, bx), np.uint8)
        st = self._lib.nus_bm_estimate(self._h, a_addr, a_len, b_addr, b_len, int(w), int(h), vec.ctypes.data, sad.ctypes.data,
                                       flags.ctypes.data)
        del ka, kb
        self._check(st)
        return vec, sad, flags

    def interpolate(self, frame_a, frame_b, w: int, h: int, *, times: Optional[Sequence[float]] = None,
                    multiplier: Optional[int] = None, mode: str = "exact", scene_detect: bool = False) -> list[bytes]:
        """Motion-compensated in-between frames of one pair (nus_bm_interpolate): at `times`, or at frame_times(multiplier).
        `scene_detect=True` runs the scene-cut detector for this call only, with the thresholds of the last set_scene_detect
        (the defaults if there was none); what set_scene_detect left on the object is not changed."""
        m = _MODE.get(str(mode).lower())
        if m is None:
            raise ValueError("mode must be 'exact' or 'fma'")
        if scene_detect and not self.scene_detect:  # on for this call, off again behind it
            self._check(self._lib.nus_bm_set_scene_detect(self._h, 1, *self._scene_thresholds))
            try:
                return self.interpolate(frame_a, frame_b, w, h, times=times, multiplier=multiplier, mode=mode)
            finally:
                self._lib.nus_bm_set_scene_detect(self._h, 0, *self._scene_thresholds)
        ts = _time_array(times, multiplier)
        n = len(ts)
        a_addr, a_len, ka = _as_buffer(frame_a)
        b_addr, b_len, kb = _as_buffer(frame_b)
        expected = int(w) * int(h) * 4
        out, oarr, oaddr = _out_buffer(expected * n)
        st = self._lib.nus_bm_interpolate(self._h, a_addr, a_len, b_addr, b_len, int(w), int(h), ts, n, m, oaddr, expected * n)
        del oarr, ka, kb
        self._check(st)
        mv = memoryview(out)
        return [bytes(mv[k * expected:(k + 1) * expected]) for k in range(n)]


class PyFrameInterpolator:
    """`PyFrameInterpolator(method="optical_flow", quality="medium")` (interpolation/mod.rs:959-1049).  "block_matching" and
    "simplified" run the block matcher at the quality's preset (name "BlockMatching"); "optical_flow" -- and, as in the reference,
    any unknown method -- is the pyramid + Horn-Schunck estimator followed by the dense-flow warp (name "OpticalFlow"; the quality
    is kept and reported).  Unknown quality strings in the constructor mean "medium"; the setter raises.  `bidirectional` (not
    in the reference) turns the block matcher's forward-backward check on; the optical-flow method has none and raises.  `flow_warps`
    (not in the reference either; 0 .. FLOW_MAX_WARPS) is the optical-flow estimator's re-linearisation rounds per finer level
    (FlowEstimator.set_warps); a block method given a non-zero value raises.  `flow_median` (0, 3 or 5; likewise) is that estimator's
    median filter behind every Jacobi run (FlowEstimator.set_median).  `flow_project` (0 .. FLOW_MAX_PROJECT; likewise) is the
    projection rounds of the optical-flow method's dense-flow warp (WgpuFrameInterpolator.set_flow_project).  `flow_bidirectional`
    (likewise) estimates every pair both ways and warps with the select warp -- each pixel takes the forward or the backward vector,
    whichever makes its two samples agree better (FlowEstimator.set_bidirectional, WgpuFrameInterpolator.interpolate_select_py); it
    is not the block matcher's `bidirectional`, and a block method given it raises; `retime` raises with it."""

    def __init__(self, method: str = "optical_flow", quality: str = "medium", *, device: int = 0, scene_detect: bool = False,
                 bidirectional: bool = False, flow_warps: int = 0, flow_median: int = 0, flow_project: int = 0,
                 flow_bidirectional: bool = False):
        from .flow import check_median, check_project, check_warps

        m = str(method).lower()
        self._scene = None  # (not in the reference) a pair flagged as a scene cut gives a repeat of the nearer frame, not a blend
        self._block = m in ("block_matching", "simplified")
        q = str(quality).lower()
        self._quality = q if q in _QUALITY else "medium"
        self._size = None
        self._device = int(device)
        if bidirectional and not self._block:
            raise ValueError("bidirectional: only the block-matching methods have a forward-backward check")
        flow_warps = check_warps(flow_warps)
        if flow_warps and self._block:
            raise ValueError("flow_warps: only the optical-flow method re-linearises its pyramid levels")
        flow_median = check_median(flow_median)
        if flow_median and self._block:
            raise ValueError("flow_median: only the optical-flow method has a flow to median-filter between its Jacobi runs")
        flow_project = check_project(flow_project)
        if flow_project and self._block:
            raise ValueError("flow_project: only the optical-flow method warps with a dense flow of its own to project")
        if flow_bidirectional and self._block:
            raise ValueError("flow_bidirectional: only the optical-flow method estimates a dense flow both ways (the block "
                             "matcher's forward-backward check is `bidirectional`)")
        self._flow_bidirectional = bool(flow_bidirectional)
        if self._block:
            self._bm = BlockMatcher(self._quality, device=device, bidirectional=bidirectional)
            if scene_detect:
                self._bm.set_scene_detect(True)
        else:
            from .flow import FlowEstimator

            self._flow = FlowEstimator(device=device, warps=flow_warps, median=flow_median, bidirectional=self._flow_bidirectional)
            if scene_detect:
                from .scene import SceneDetector

                self._scene = SceneDetector(device=device)
            self._warp = WgpuFrameInterpolator(device=device)
            if flow_project:
                self._warp.set_flow_project(flow_project)

    def retime(self, frames, fps_in, fps_out) -> list[bytes]:
        """A list of host frames of the initialize() size converted from `fps_in` to `fps_out` (ints or Fractions; retime.py has the
        schedule): a list of host frames, real frames where the output grid meets one, else the method's in-between frame of the
        pair at the schedule's time -- the frame `interpolate` returns for it, scene detection included.  One upload, the device
        entry points (retime.retime_frames), one download; the bytes travel through `transfer`."""
        from .retime import retime_frames

        if self._size is None:
            raise RuntimeError("Interpolator not initialized")
        w, h = self._size
        frames = list(frames)
        if any(len(memoryview(f).cast("B")) != w * h * 4 for f in frames):
            raise RuntimeError("Frame size mismatch")
        if self._flow_bidirectional:  # the library's refusal (ValueError with its text), before any GPU work
            self._flow.retime_device_stream(0, len(frames), w, h, 1, 1, 0)
        if self._block:
            return retime_frames(frames, w, h, fps_in, fps_out, matcher=self._bm, device=self._device)
        return retime_frames(frames, w, h, fps_in, fps_out, warp=self._warp, flow=self._flow, scene=self._scene, device=self._device)

    @staticmethod
    def create_best_interpolator(quality: str = "medium") -> "PyFrameInterpolator":
        return PyFrameInterpolator("optical_flow", quality)  # :927-930: "For now, use optical flow as best method"

    def initialize(self, width: int, height: int) -> None:
        w, h = int(width), int(height)
        if w <= 0 or h <= 0 or w * h >= 1 << 31:
            raise RuntimeError("initialize: bad dimensions")
        self._size = (w, h)

    def interpolate(self, frame1, frame2, t: float) -> bytes:
        if self._size is None:
            raise RuntimeError("Interpolator not initialized")
        w, h = self._size
        if len(memoryview(frame1).cast("B")) != w * h * 4 or len(memoryview(frame2).cast("B")) != w * h * 4:
            raise RuntimeError("Frame size mismatch")
        if self._block:
            try:
                return self._bm.interpolate(frame1, frame2, w, h, times=[t])[0]
            except ValueError as e:  # the pyclass raises PyRuntimeError for everything (:1011-1019)
                raise RuntimeError(str(e)) from e
        if self._scene is not None and self._scene.detect(frame1, frame2, w, h)[0]:
            return self._warp.interpolate_py(frame1, frame2, w, h, time_t=0.0 if float(t) < 0.5 else 1.0)
        flow = self._flow.estimate(frame1, frame2, w, h)
        if self._flow_bidirectional:
            return self._warp.interpolate_select_py(frame1, frame2, w, h, flow, self._flow.estimate(frame2, frame1, w, h), time_t=float(t))
        return self._warp.interpolate_py(frame1, frame2, w, h, time_t=float(t), flow=flow)

    @property
    def name(self) -> str:
        return "BlockMatching" if self._block else "OpticalFlow"

    @property
    def quality(self) -> str:
        return self._quality

    @quality.setter
    def quality(self, quality: str) -> None:
        q = str(quality).lower()
        if q not in _QUALITY:
            raise ValueError("Invalid quality setting")
        if self._block:
            self._bm.set_quality(q)
        self._quality = q
