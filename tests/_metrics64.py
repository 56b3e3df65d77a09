"""The float64 definition of the image-quality metrics the library computes (include/nuscaler_hip.h, nus_metrics_*), in numpy:
the yardstick of tests/test_gpu_metrics.py.  Test infrastructure only; the product never imports it.

MSE / PSNR are ErrorMetrics::calculate (Nu_scale/src/upscale/common.rs:494-519).  SSIM is Wang et al. 2004 per channel on
0..255 with an 11 x 11 Gaussian window (sigma 1.5, normalised), population statistics and the valid centres only -- what
skimage.metrics.structural_similarity(a, b, channel_axis=2, gaussian_weights=True, sigma=1.5, use_sample_covariance=False,
data_range=255) computes on R, G, B.

ssim_kernel_model restates what k_metrics_ssim (nus_k_metrics.hip) computes per window, rounding by rounding, so that the distance
between the kernel's arithmetic and the definition can be measured without a GPU (tests/test_metrics_reference.py)."""
import math

import numpy as np
from scipy.ndimage import correlate1d

C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2
RADIUS = 5


def gaussian_weights():
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2 * 1.5 ** 2))
    return g / g.sum()


def sse(a, b) -> int:
    d = a[..., :3].astype(np.int64) - b[..., :3].astype(np.int64)
    return int((d * d).sum())


def mse(a, b) -> float:
    h, w = a.shape[:2]
    return sse(a, b) / (float(w * h) * 3.0)


def psnr_of(m: float) -> float:
    return 20.0 * math.log10(255.0 / math.sqrt(m)) if m > 0.0 else math.inf


def _filt(x, g):
    """Separable window sums at the valid centres only."""
    y = correlate1d(correlate1d(x, g, axis=0, mode="constant"), g, axis=1, mode="constant")
    return y[RADIUS:-RADIUS, RADIUS:-RADIUS]


def ssim_map(x, y):
    """Per-centre SSIM of one channel (float64 arrays of one shape), valid centres only."""
    g = gaussian_weights()
    mx, my = _filt(x, g), _filt(y, g)
    sxx = _filt(x * x, g) - mx * mx
    syy = _filt(y * y, g) - my * my
    sxy = _filt(x * y, g) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def ssim(a, b) -> float:
    h, w = a.shape[:2]
    if w < 2 * RADIUS + 1 or h < 2 * RADIUS + 1:
        return math.nan
    total = 0.0
    for c in range(3):
        total += float(ssim_map(a[..., c].astype(np.float64), b[..., c].astype(np.float64)).sum())
    return total / (3.0 * (w - 2 * RADIUS) * (h - 2 * RADIUS))


# the kernel's window: the float64 weights rounded to f32 (kG of nus_k_metrics.hip, taps -5..0; symmetric)
KG = np.array([float.fromhex(v) for v in ("0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c40p-3",
                                          "0x1.106560p-2")], dtype=np.float32)
KG11 = np.concatenate([KG, KG[4::-1]])


def _fma32(g, v, acc):
    """fmaf on f32 arrays: the 48-bit product is exact in f64; the sum rounds to f64 and then to f32 (a double rounding that
    differs from fmaf in about one case in 2^29, far below anything measured here)."""
    return (np.float64(g) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _window_passes(v, dtype):
    """The kernel's two 11-tap passes over (..., H, W): horizontal, then vertical, taps in the order 0..10, one FMA per tap."""
    w, h = v.shape[-1], v.shape[-2]
    for axis, n in ((-1, w - 2 * RADIUS), (-2, h - 2 * RADIUS)):
        acc = np.zeros(v.shape[:axis] + (n,) + (v.shape[axis + 1:] if axis != -1 else ()), dtype)
        for tp in range(2 * RADIUS + 1):
            tap = v[..., tp:tp + n] if axis == -1 else v[..., tp:tp + n, :]
            # f64: the horizontal sums are exact (24-bit weights, integers below 2^16) and the vertical FMAs round at 2^-53; a
            # multiply and an add in their place moves a window's SSIM by 1e-13 at most
            acc = _fma32(KG11[tp], tap, acc) if dtype == np.float32 else np.float64(KG11[tp]) * tap + acc
        v = acc
    return v


def ssim_kernel_model(a, b, parent=False):
    """k_metrics_ssim in numpy, for one pair of (H, W, 4) uint8 frames or a batch (N, H, W, 4): -> SSIM, a float or (N,) float64.
      now:    the pixels as they are; x, y, x^2, y^2, xy through both passes in f64 with the f32 weights; the differences
              E[x^2] - mx^2, E[y^2] - my^2, E[xy] - mx*my in f64; these three and the two means rounded to f32 once; the ratio in
              f32, unfused, in the kernel's order; the windows' ratios added in f64.
      parent: the kernel before that: x - 128, everything in f32 (FMA per tap), the three differences in f32 from a rounded
              product, the means shifted back by 128 in f32.  Kept so that its distance to the definition stays reproducible."""
    a, b = np.asarray(a), np.asarray(b)
    single = a.ndim == 3
    if single:
        a, b = a[None], b[None]
    h, w = a.shape[1:3]
    f32 = np.float32
    dtype = f32 if parent else np.float64
    total = np.zeros(a.shape[0], np.float64)
    for c in range(3):
        x, y = a[..., c].astype(dtype), b[..., c].astype(dtype)
        if parent:
            x, y = x - f32(128), y - f32(128)
        mx, my = _window_passes(x, dtype), _window_passes(y, dtype)
        sxx = _window_passes(x * x, dtype) - mx * mx
        syy = _window_passes(y * y, dtype) - my * my
        sxy = _window_passes(x * y, dtype) - mx * my
        if parent:
            mx, my = mx + f32(128), my + f32(128)
        else:
            mx, my, sxx, syy, sxy = (v.astype(f32) for v in (mx, my, sxx, syy, sxy))
        num = (f32(2) * mx * my + f32(C1)) * (f32(2) * sxy + f32(C2))
        den = (mx * mx + my * my + f32(C1)) * (sxx + syy + f32(C2))
        assert num.dtype == f32 and den.dtype == f32
        total += (num / den).astype(np.float64).sum(axis=(1, 2))
    out = total / (3.0 * (w - 2 * RADIUS) * (h - 2 * RADIUS))
    return float(out[0]) if single else out


def metrics(a, b):
    """(mse, psnr, ssim) of two (H, W, 4) uint8 frames; ssim NaN below 11 x 11."""
    m = mse(a, b)
    return m, psnr_of(m), ssim(a, b)
