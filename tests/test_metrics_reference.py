"""Pins tests/_metrics64.py, the float64 yardstick of the GPU metrics: against a brute-force window loop, closed forms, the
reference's sequential MSE sum (Nu_scale/src/upscale/common.rs:494-511), and alpha."""
import math

import numpy as np
import pytest

import _metrics64 as M64


def _brute_ssim(a, b):
    g = M64.gaussian_weights()
    win = np.outer(g, g)
    h, w = a.shape[:2]
    total, count = 0.0, 0
    for c in range(3):
        x_all, y_all = a[..., c].astype(np.float64), b[..., c].astype(np.float64)
        for cy in range(5, h - 5):
            for cx in range(5, w - 5):
                x = x_all[cy - 5:cy + 6, cx - 5:cx + 6]
                y = y_all[cy - 5:cy + 6, cx - 5:cx + 6]
                mx, my = (win * x).sum(), (win * y).sum()
                sxx = (win * x * x).sum() - mx * mx
                syy = (win * y * y).sum() - my * my
                sxy = (win * x * y).sum() - mx * my
                total += ((2 * mx * my + M64.C1) * (2 * sxy + M64.C2)) / ((mx * mx + my * my + M64.C1) * (sxx + syy + M64.C2))
                count += 1
    return total / count


@pytest.mark.parametrize("shape", [(13, 12), (16, 11), (11, 11)])
def test_separable_form_equals_brute_force(shape):
    w, h = shape
    rng = np.random.default_rng(w * h)
    a = rng.integers(0, 256, (h, w, 4), dtype=np.int32).astype(np.uint8)
    b = np.clip(a.astype(np.int32) + rng.integers(-40, 41, (h, w, 4)), 0, 255).astype(np.uint8)
    assert abs(M64.ssim(a, b) - _brute_ssim(a, b)) <= 1e-12


def test_window_is_the_normalised_gaussian():
    g = M64.gaussian_weights()
    assert len(g) == 11 and abs(g.sum() - 1.0) < 1e-15 and np.allclose(g, g[::-1])
    assert abs(g[6] / g[5] - math.exp(-1 / (2 * 1.5 ** 2))) < 1e-15


def test_identical_frames():
    a = np.random.default_rng(1).integers(0, 256, (20, 17, 4), dtype=np.int32).astype(np.uint8)
    m, p, s = M64.metrics(a, a)
    assert m == 0.0 and p == math.inf and s == pytest.approx(1.0, abs=1e-15)


@pytest.mark.parametrize("c1,c2", [(0, 255), (250, 251), (100, 100), (17, 200)])
def test_constant_frames_closed_form(c1, c2):
    a = np.full((14, 15, 4), c1, np.uint8)
    b = np.full((14, 15, 4), c2, np.uint8)
    want = (2 * c1 * c2 + M64.C1) / (c1 * c1 + c2 * c2 + M64.C1)
    assert M64.ssim(a, b) == pytest.approx(want, abs=1e-12)
    assert M64.mse(a, b) == float((c1 - c2) ** 2)


def test_mse_equals_the_reference_sequential_sum():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (9, 23, 4), dtype=np.int32).astype(np.uint8)
    b = rng.integers(0, 256, (9, 23, 4), dtype=np.int32).astype(np.uint8)
    h, w = a.shape[:2]
    s = 0.0  # common.rs:497-509, in its order
    for y in range(h):
        for x in range(w):
            for c in range(3):
                d = int(a[y, x, c]) - int(b[y, x, c])
                s += float(d * d)
    want = s / (float(w * h) * 3.0)
    assert M64.mse(a, b) == want
    assert M64.psnr_of(want) == 20.0 * math.log10(255.0 / math.sqrt(want))


def test_alpha_has_no_effect():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (15, 18, 4), dtype=np.int32).astype(np.uint8)
    b = rng.integers(0, 256, (15, 18, 4), dtype=np.int32).astype(np.uint8)
    a2, b2 = a.copy(), b.copy()
    a2[..., 3], b2[..., 3] = 0, 255
    assert M64.metrics(a, b) == M64.metrics(a2, b2)


def test_ssim_is_nan_below_eleven_pixels():
    a = np.zeros((10, 40, 4), np.uint8)
    assert math.isnan(M64.ssim(a, a)) and M64.mse(a, a) == 0.0
