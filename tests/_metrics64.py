"""The float64 definition of the image-quality metrics the library computes (include/nuscaler_hip.h, nus_metrics_*), in numpy:
the yardstick of tests/test_gpu_metrics.py.  Test infrastructure only; the product never imports it.

MSE / PSNR are ErrorMetrics::calculate (Nu_scale/src/upscale/common.rs:494-519).  SSIM is Wang et al. 2004 per channel on
0..255 with an 11 x 11 Gaussian window (sigma 1.5, normalised), population statistics and the valid centres only -- what
skimage.metrics.structural_similarity(a, b, channel_axis=2, gaussian_weights=True, sigma=1.5, use_sample_covariance=False,
data_range=255) computes on R, G, B."""
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


def metrics(a, b):
    """(mse, psnr, ssim) of two (H, W, 4) uint8 frames; ssim NaN below 11 x 11."""
    m = mse(a, b)
    return m, psnr_of(m), ssim(a, b)
