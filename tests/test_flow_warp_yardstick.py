"""The yardstick of the flow estimator's re-linearisation mode, checked on the CPU (tests/_flow_warp64.py): the float64 witness
with warps = 0 is tests/_flow64.py's estimator; on the scenes with a rendered true mid-frame one round per finer level buys what
DESIGN section 8.1 says it buys; the float32 restatement of the stage stays within the tolerance the GPU tests use, and a wrong
sampler or a wrong It' does not."""
import numpy as np
import pytest

import _flow64 as F
import _flow_warp64 as W
import oracle

WIDE = [r for r in W.ROWS if r[0] >= 192]
CROP = (67, 45)  # of ROWS[0]: the small size of tests/test_gpu_flow_warp.py


@pytest.fixture(scope="module")
def table():
    return [(row, W.table_row(oracle.warp_blend, row)) for row in W.ROWS]


def test_rows_are_the_issue_scenes():
    assert len(W.ROWS) == 7 and len(WIDE) == 6


def test_warps_zero_is_the_flow64_estimator():
    a, b, _ = W.scene(W.ROWS[4])
    assert np.array_equal(W.estimate(a, b, warps=0, **W.PARAMS), F.estimate(a, b, **W.PARAMS))
    a, b = a[:45, :67], b[:45, :67]  # odd sizes at every level
    assert np.array_equal(W.estimate(a, b, 4, 7, 3, 4e-4, warps=0), F.estimate(a, b, 4, 7, 3, 4e-4))
    # no refining steps: a round has nothing to run, whatever warps says
    assert np.array_equal(W.estimate(a, b, 3, 5, 0, 4e-4, warps=2), F.estimate(a, b, 3, 5, 0, 4e-4))


def test_quality_table(table):
    print("\n" + W.format_table(table))
    for row, (zero, w0, w1, w2) in table:
        print(f"{row}: warps 1 - warps 0 = {w1 - w0:+.2f} dB, warps 2 - warps 1 = {w2 - w1:+.2f} dB")
    for row, (zero, w0, w1, w2) in table:
        assert w1 >= w0 + 0.5, (row, w0, w1)
        if row[0] >= 192:
            assert w1 >= w0 + 2.0, (row, w0, w1)
        assert w2 >= w1 - 0.5, (row, w1, w2)


def _cases():
    out = [(row, W.scene(row)[:2]) for row in W.ROWS]
    a, b, _ = W.scene(W.ROWS[0])
    out.append((CROP, (a[:CROP[1], :CROP[0]].copy(), b[:CROP[1], :CROP[0]].copy())))
    return out


@pytest.mark.parametrize("warps", [1, 2])
def test_float32_restatement_within_tolerance_and_wrong_variants_beyond(warps):
    worst = 0.0
    for name, (a, b) in _cases():
        f32 = W.estimate_f32(oracle, a, b, warps=warps, **W.PARAMS)
        assert f32.dtype == np.float32
        d = float(np.abs(f32 - W.estimate(a, b, warps=warps, **W.PARAMS)).max())
        d_nearest = float(np.abs(f32 - W.estimate(a, b, warps=warps, nearest=True, **W.PARAMS)).max())
        d_linear = float(np.abs(f32 - W.estimate(a, b, warps=warps, linear_terms=False, **W.PARAMS)).max())
        print(f"{name} warps {warps}: |f32 - f64| = {d:.3g} px; nearest sampling {d_nearest:.3g}; It' without Ix u0 + Iy v0 {d_linear:.3g}")
        worst = max(worst, d)
        assert d <= W.F32_TOLERANCE, (name, d)
        assert d_nearest > W.F32_TOLERANCE and d_linear > W.F32_TOLERANCE, (name, d_nearest, d_linear)
    print(f"warps {warps}: largest |f32 - f64| = {worst:.3g} px, recorded maximum {W.F32_MEASURED_MAX:.3g}, tolerance {W.F32_TOLERANCE:.3g}")
    assert worst <= W.F32_MEASURED_MAX  # the recorded figure is the measured maximum, rounded up


def test_float32_stage_with_zero_flow_is_todays_triple():
    rng = np.random.default_rng(5)
    i1, i2 = rng.random((9, 13, 4), np.float32), rng.random((9, 13, 4), np.float32)
    c0 = W.coefficients_f32(i1, i2, None)
    cz = W.coefficients_f32(i1, i2, np.zeros((9, 13, 2), np.float32))
    assert np.array_equal(c0, cz)
    assert np.array_equal(c0[..., 2], W.luminance_f32(i2) - W.luminance_f32(i1))
    # and its Jacobi steps are the oracle's horn_schunck
    for start in (None, (rng.random((9, 13, 2), np.float32) - 0.5) * 3):
        assert np.array_equal(W.jacobi_coef_f32(c0, start, 4, 4e-4), oracle.horn_schunck(i1, i2, start, 4, 4e-4))


def test_stage_float32_against_float64():
    """The stage alone: (Ix, Iy, It') in float32 against float64 on the same f32 inputs, flows up to +-12 px."""
    rng = np.random.default_rng(6)
    i1, i2 = rng.random((45, 67, 4), np.float32), rng.random((45, 67, 4), np.float32)
    flow = ((rng.random((45, 67, 2)) - 0.5) * 24).astype(np.float32)
    c32 = W.coefficients_f32(i1, i2, flow)
    ix, iy, it = W.coefficients(F.luminance(i1), F.luminance(i2), flow.astype(np.float64))
    d = float(np.abs(c32 - np.stack([ix, iy, it], -1)).max())
    print(f"stage: |f32 - f64| = {d:.3g}")
    # operands below 1 and 12: It' sums four terms of at most 1 + 1 + 6 + 6, each rounded at 2^-24 relative, a few times over
    assert d <= 14 * 8 * 2.0 ** -24
