"""Image-quality metrics on the HIP device: the reference's `ErrorMetrics` (Nu_scale/src/upscale/common.rs:475-543) -- MSE and
PSNR over R, G, B -- with a real SSIM where the reference keeps a 0.0 placeholder.  Bound to `nus_metrics_*` of
include/nuscaler_hip.h; the definitions are written there.  Alpha is ignored.  No torch type crosses into this module: the
device entry point takes integer device addresses, as `WgpuFrameInterpolator.interpolate_device` does.

SSIM is what `skimage.metrics.structural_similarity(a, b, channel_axis=2, gaussian_weights=True, sigma=1.5,
use_sample_covariance=False, data_range=255)` computes on the RGB channels."""
from __future__ import annotations

import ctypes
import math

from . import _capi as C

SSIM_MIN_SIDE = 11  # the 11 x 11 window must fit


def _mask(mse: bool, ssim: bool) -> int:
    return (C.METRIC_MSE if mse else 0) | (C.METRIC_SSIM if ssim else 0)


def workspace_size(w: int, h: int, frames: int, mse: bool = True, ssim: bool = True) -> int:
    """Bytes of device workspace `compare_device` needs (nus_metrics_workspace_size); ValueError for an invalid shape."""
    n = int(C.lib().nus_metrics_workspace_size(int(w), int(h), int(frames), _mask(mse, ssim)))
    if n == 0:
        raise ValueError(C.last_error())
    return n


def compare_device(d_a: int, a_stride: int, d_b: int, b_stride: int, w: int, h: int, frames: int, d_workspace: int,
                   workspace_bytes: int, d_out: int, *, mse: bool = True, ssim: bool = True, stream: int = 0) -> None:
    """Enqueue the metrics of `frames` pairs on `stream`: frame i of A at d_a + i * a_stride, of B at d_b + i * b_stride; the
    device buffer at d_out receives 3 float64 per frame, [mse, psnr, ssim] (NaN for what was not asked)."""
    st = C.lib().nus_metrics_compare_device(d_a or None, int(a_stride), d_b or None, int(b_stride), int(w), int(h), int(frames),
                                            _mask(mse, ssim), d_workspace or None, int(workspace_bytes), d_out or None,
                                            stream or None)
    if st != C.OK:
        msg = C.last_error()
        raise ValueError(msg) if st in (C.ERR_INVALID_ARGUMENT, C.ERR_SIZE_MISMATCH) else RuntimeError(msg)


class ErrorMetrics:
    """`ErrorMetrics` (common.rs:475-543): `ErrorMetrics.calculate(upscaled, reference)`, then the accessors `mse()`, `psnr()`
    and `ssim()`.  SSIM is NaN for frames smaller than 11 x 11 (the reference always reported 0.0)."""

    __slots__ = ("_mse", "_psnr", "_ssim")

    def __init__(self, mse: float, psnr: float, ssim: float):
        self._mse, self._psnr, self._ssim = float(mse), float(psnr), float(ssim)

    @classmethod
    def calculate(cls, upscaled, reference, *, device: int = 0) -> "ErrorMetrics":
        """Two uint8 numpy arrays of shape (H, W, 4), RGBA8 (or any channel order the two share)."""
        import numpy as np

        a, b = np.asarray(upscaled), np.asarray(reference)
        if a.shape != b.shape:
            raise ValueError("Images must have the same dimensions")  # common.rs:486-488
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or b.dtype != np.uint8:
            raise ValueError("ErrorMetrics.calculate: expected two uint8 arrays of shape (H, W, 4)")
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        h, w = int(a.shape[0]), int(a.shape[1])
        ssim = w >= SSIM_MIN_SIDE and h >= SSIM_MIN_SIDE
        out = (ctypes.c_double * 3)()
        st = C.lib().nus_metrics_compare(int(device), a.ctypes.data, a.nbytes, b.ctypes.data, b.nbytes, w, h, _mask(True, ssim),
                                         out)
        if st != C.OK:
            msg = C.last_error()
            raise ValueError(msg) if st in (C.ERR_INVALID_ARGUMENT, C.ERR_SIZE_MISMATCH) else RuntimeError(msg)
        return cls(out[0], out[1], out[2] if ssim else math.nan)

    def mse(self) -> float:
        return self._mse

    def psnr(self) -> float:
        return self._psnr

    def ssim(self) -> float:
        return self._ssim

    def line(self) -> str:
        """The line both command-line tools print: mse=.. psnr=.. ssim=.. (six decimals; inf / nan where they apply)."""
        return f"mse={self._mse:.6f} psnr={self._psnr:.6f} ssim={self._ssim:.6f}"

    def __repr__(self) -> str:
        return f"ErrorMetrics({self.line()})"
