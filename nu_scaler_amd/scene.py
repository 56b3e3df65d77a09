"""Scene-cut detection of frame pairs on the HIP device and the cut-aware output rule, bound to `nus_scene_*` of
include/nuscaler_hip.h (the contract is written there).  Build-defined: the reference interpolates every pair of a stream.
The thresholds' defaults are settings, not measurements.  No torch type crosses into this module: the device entry points
take integer device addresses, as `BlockMatcher.estimate_device` does."""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from . import _capi as C
from .upscaler import _as_buffer

_FORMAT = {"rgba": C.FORMAT_RGBA8, "bgra": C.FORMAT_BGRA8, "rgbx": C.FORMAT_RGBX8, "bgrx": C.FORMAT_BGRX8}
MEASURES_DTYPE = np.dtype([("sad", "<u8"), ("hist_l1", "<u4"), ("reserved", "<u4")])  # nus_scene_measures


def pixel_format(fmt) -> int:
    """nus_pixel_format of "rgba" / "bgra" / "rgbx" / "bgrx" (or the integer itself)."""
    if isinstance(fmt, str):
        f = _FORMAT.get(fmt.lower())
        if f is None:
            raise ValueError("pixel format must be 'rgba', 'bgra', 'rgbx' or 'bgrx'")
        return f
    if isinstance(fmt, bool) or not isinstance(fmt, (int, np.integer)) or not 0 <= int(fmt) <= 3:
        raise ValueError(f"unknown pixel format {fmt!r}")
    return int(fmt)


def check_thresholds(mad_threshold, hist_permille) -> tuple[int, int]:
    """The detector's two settings as integers; ValueError outside 0 .. 255 / 0 .. 1000."""
    for name, v, hi in (("mad_threshold", mad_threshold, 255), ("hist_permille", hist_permille, 1000)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer from 0 to {hi}, got {v!r}")
    return int(mad_threshold), int(hist_permille)


def _check(status: int) -> None:
    if status == C.OK:
        return
    msg = C.last_error()
    raise ValueError(msg) if status in (C.ERR_INVALID_ARGUMENT, C.ERR_SIZE_MISMATCH) else RuntimeError(msg)


class SceneDetector:
    """cut  <=>  sad >= mad_threshold * 3 W H  and  hist_l1 * 1000 >= hist_permille * 2 W H  (integers; include/nuscaler_hip.h)."""

    def __init__(self, mad_threshold: int = C.SCENE_DEFAULT_MAD, hist_permille: int = C.SCENE_DEFAULT_HIST_PERMILLE, device: int = 0):
        self.mad_threshold, self.hist_permille = check_thresholds(mad_threshold, hist_permille)
        self.device = int(device)
        self._lib = C.lib()

    @staticmethod
    def workspace_size(w: int, h: int, n_pairs: int = 1) -> int:
        """Bytes of device workspace `detect_device` needs (nus_scene_workspace_size); ValueError for an invalid shape."""
        n = int(C.lib().nus_scene_workspace_size(int(w), int(h), int(n_pairs)))
        if n == 0:
            raise ValueError(C.last_error())
        return n

    def detect(self, frame_a, frame_b, w: int, h: int, fmt="rgba") -> tuple[bool, int, int]:
        """One host pair (bytes or uint8 arrays) -> (cut, sad, hist_l1)."""
        a_addr, a_len, ka = _as_buffer(frame_a)
        b_addr, b_len, kb = _as_buffer(frame_b)
        meas = np.zeros(1, MEASURES_DTYPE)
        cut = ctypes.c_uint8(0)
        st = self._lib.nus_scene_detect(self.device, a_addr, a_len, b_addr, b_len, int(w), int(h), pixel_format(fmt), self.mad_threshold,
                                        self.hist_permille, meas.ctypes.data, ctypes.addressof(cut))
        del ka, kb
        _check(st)
        return bool(cut.value), int(meas["sad"][0]), int(meas["hist_l1"][0])

    def detect_device(self, d_a: int, a_stride: int, d_b: int, b_stride: int, w: int, h: int, n_pairs: int, d_workspace: int,
                      workspace_bytes: int, d_cut: int, d_measures: int = 0, fmt="rgba", stream: int = 0) -> None:
        """Enqueue the detection of `n_pairs` pairs on `stream` (nus_scene_detect_device): one u8 per pair at d_cut, a
        nus_scene_measures (MEASURES_DTYPE) per pair at d_measures (0: not wanted)."""
        _check(self._lib.nus_scene_detect_device(d_a or None, int(a_stride), d_b or None, int(b_stride), int(w), int(h), int(n_pairs),
                                                 pixel_format(fmt), self.mad_threshold, self.hist_permille, d_workspace or None,
                                                 int(workspace_bytes), d_measures or None, d_cut or None, stream or None))

    def apply_cuts_device(self, d_a: int, a_stride: int, d_b: int, b_stride: int, w: int, h: int, times: Sequence[float], d_cut: int,
                          d_out: int, out_pair_stride: int = 0, n_pairs: int = 1, fmt="rgba", stream: int = 0) -> None:
        """Enqueue the cut-aware output rule behind a multi-time interpolation (nus_scene_apply_cuts_device): the frames of every
        pair with a non-zero flag become repeats of A (time < 0.5) or B; other pairs are not touched."""
        ts = (ctypes.c_float * len(times))(*[float(t) for t in times])
        _check(self._lib.nus_scene_apply_cuts_device(d_a or None, int(a_stride), d_b or None, int(b_stride), int(w), int(h),
                                                     pixel_format(fmt), ts, len(times), d_cut or None, d_out or None,
                                                     int(out_pair_stride), int(n_pairs), stream or None))
