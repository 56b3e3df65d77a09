"""Pins tests/_metrics64.py, the float64 yardstick of the GPU metrics: against a brute-force window loop, closed forms, the
reference's sequential MSE sum (Nu_scale/src/upscale/common.rs:494-511), and alpha.  Then ssim_kernel_model, the restatement of
k_metrics_ssim's arithmetic, on the adversarial frames of tests/_metrics_cases.py: the arithmetic the kernel had before (f32
throughout) misses the 1e-5 contract on flat frames by a known amount, the present one (f64 statistics and differences, f32
ratio) stays within _metrics_cases.SSIM_TOL, and identical frames give exactly 1."""
import math

import numpy as np
import pytest

import _metrics64 as M64
import _metrics_cases as MC


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


# ---- the kernel's arithmetic, restated (ssim_kernel_model) against the definition --------------------------------------------------
def _model_error(name, parent=False):
    A, B = MC.batch(name)
    return np.abs(M64.ssim_kernel_model(A, B, parent=parent) - MC.witness(name))


def test_there_are_1015_constant_pairs():
    cd = MC.constant_pair_levels()
    assert len(cd) == 1015 == len(set(cd)) and all(0 <= c <= 255 and 0 <= d <= 255 and c != d for c, d in cd)


def test_model_weights_are_the_f32_roundings_of_the_window():
    assert np.array_equal(M64.KG11, M64.gaussian_weights().astype(np.float32)) and M64.KG11.dtype == np.float32


def test_parent_arithmetic_misses_the_contract_on_constant_pairs():
    """f32 statistics and an f32 E[x^2] - mu^2: 445 of the 1015 constant pairs miss 1e-5, the worst (235 against 234, 22 against
    21, 229 against 227) by 1.17e-4.  Asserted within a factor of 2, so that this documents the defect and not a guess."""
    err = _model_error("constant", parent=True)
    print(f"parent arithmetic, constant pairs: worst {err.max():.3e}, {(err > 1e-5).sum()} of {len(err)} above 1e-5")
    assert 1.17e-4 / 2 <= err.max() <= 1.17e-4 * 2, err.max()
    assert (err > 1e-5).sum() >= 400
    worst = {MC.constant_pair_levels()[i] for i in np.flatnonzero(err >= 0.99 * err.max())}
    assert worst & {(235, 234), (22, 21), (229, 227)}, worst
    # a 16/17 letterbox black, and the per-channel sweep
    assert err[MC.constant_pair_levels().index((16, 17))] > 1e-5
    assert _model_error("constant_rgb", parent=True).max() > 1e-5


def test_parent_arithmetic_misses_the_new_tolerance_on_stripes_and_letterbox():
    for name in ("periodic_30x28", "letterbox", "pillarbox"):
        err = _model_error(name, parent=True)
        print(f"parent arithmetic, {name}: worst {err.max():.3e}")
        assert err.max() > MC.SSIM_TOL, (name, err.max())
    assert _model_error("periodic_30x28", parent=True).max() > 1e-5


@pytest.mark.parametrize("name", MC.BATCHES)
def test_kernel_arithmetic_stays_within_the_asserted_tolerance(name):
    """The measured worst case over every class (and over the SHAPES x CONTENTS of tests/test_gpu_metrics.py, up to 3840 x 2160) is
    _metrics_cases.SSIM_MODEL_WORST; the tolerance the GPU tests assert is 4 x that, and it is below the public 1e-5."""
    err = _model_error(name)
    print(f"kernel arithmetic, {name}: worst {err.max():.3e} over {len(err)} pairs")
    assert err.max() <= MC.SSIM_MODEL_WORST, (name, err.max())
    assert MC.SSIM_TOL == 4 * MC.SSIM_MODEL_WORST <= 1e-5


@pytest.mark.parametrize("name", MC.BATCHES)
def test_model_gives_exactly_one_on_identical_frames(name):
    A, B = MC.batch(name)
    for frames in (A, B):
        assert np.all(M64.ssim_kernel_model(frames, frames) == 1.0)
    assert M64.ssim_kernel_model(A[0], A[0]) == 1.0 and isinstance(M64.ssim_kernel_model(A[0], B[0]), float)
