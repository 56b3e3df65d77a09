"""The yardstick of the flow estimator's re-linearisation mode, checked on the CPU (tests/_flow_warp64.py): the float64 witness
with warps = 0 is tests/_flow64.py's estimator; on the scenes with a rendered true mid-frame one round per finer level buys what
DESIGN section 8.1 says it buys; the float32 restatement of the stage stays within the tolerance the GPU tests use, and a wrong
sampler or a wrong It' does not.  The same for the lattice of settings tests/test_gpu_flow_warp_lattice.py runs (W.LATTICE: level
counts 1 .. 4, step counts that split unevenly, 0 steps, warps 1 .. 4): every figure printed, the largest recorded."""
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


# ---- the lattice of settings (W.LATTICE) ----------------------------------------------------------------------------------------------
def _lattice_figure(case, warps, **wrong):
    w, h, levels, coarse, refine = case
    a, b = W.lattice_frames(w, h)
    f32 = W.estimate_f32(oracle, a, b, levels, coarse, refine, W.LATTICE_LAMBDA, warps=warps)
    assert f32.dtype == np.float32 and f32.shape == (h, w, 2)
    return float(np.abs(f32 - W.estimate(a, b, levels, coarse, refine, W.LATTICE_LAMBDA, warps=warps, **wrong)).max())


def test_lattice_holds_what_it_must():
    """The table may grow, not shrink below this."""
    cases = W.LATTICE
    assert len(set(cases)) == len(cases)
    assert {c[2] for c in cases} >= {1, 2, 3, 4}
    assert any(c[3] == 0 and c[4] > 0 for c in cases) and any(c[4] == 0 and c[3] > 0 for c in cases)
    refine = {c[4] for c in cases}
    assert 1 in refine and 13 in refine and refine & {6, 7}
    assert {129, 257} <= {c[1] for c in cases}
    assert any(c[0] > 162 for c in cases)
    assert any(c[:2] == (613, 517) for c in cases) and any(c[:2] == (2, 2) for c in cases) and any(c[:2] == (1, 1) for c in cases)
    assert max(c[0] * c[1] for c in cases) == 613 * 517  # no larger shape than that
    assert W.LATTICE_LAMBDA == 4e-4


def test_lattice_frames_are_the_scene_crop_and_cyclic():
    import _bm_bidir as scenes

    w, h = 67, 45
    a, b, _ = scenes.scene(w + 64, h + 64, (-2, 1), (6, 4), 24)
    fr = W.lattice_frames(w, h, 18)
    assert fr.shape == (18, h, w, 4) and fr.dtype == np.uint8 and fr.flags["C_CONTIGUOUS"]
    assert np.array_equal(fr[0], a[16:16 + h, 24:24 + w]) and np.array_equal(fr[1], b[16:16 + h, 24:24 + w])
    assert np.array_equal(fr[:2], W.lattice_frames(w, h))
    assert np.array_equal(fr[8:16], fr[:8]) and np.array_equal(fr[16:], fr[:2])
    pairs = {(fr[k].tobytes(), fr[k + 1].tobytes()) for k in range(8)}
    assert len(pairs) == 8  # 8 distinct consecutive pairs, the wrap from frame 7 to frame 0 among them
    small = W.lattice_frames(5, 3)
    rng = np.random.default_rng(503)
    assert small.shape == (2, 3, 5, 4) and np.array_equal(small, rng.integers(0, 256, (2, 3, 5, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        W.lattice_frames(5, 3, 3)


_lattice_worst = {}


@pytest.mark.parametrize("warps", [1, 2, 3, 4])
def test_lattice_float32_restatement_within_tolerance(warps):
    worst = 0.0
    for case in W.LATTICE:
        d = _lattice_figure(case, warps)
        print(f"{W.lattice_id(case)} warps {warps}: |f32 - f64| = {d:.3g} px")
        worst = max(worst, d)
        assert d <= W.F32_TOLERANCE, (case, warps, d)
    print(f"warps {warps}: largest |f32 - f64| = {worst:.3g} px, recorded maximum {W.F32_LATTICE_MEASURED_MAX:.3g}, tolerance {W.F32_TOLERANCE:.3g}")
    assert worst <= W.F32_LATTICE_MEASURED_MAX
    _lattice_worst[warps] = worst
    if len(_lattice_worst) == 4:  # the recorded figure is the measured maximum, rounded up: at most one unit of its second digit above
        assert W.F32_LATTICE_MEASURED_MAX - 0.2e-4 <= max(_lattice_worst.values()) <= W.F32_LATTICE_MEASURED_MAX


def test_lattice_cases_without_a_round_are_the_warps_zero_witness():
    """refine_iters = 0 and one level: there is nothing to re-linearise, whatever warps says."""
    none = [c for c in W.LATTICE if c[4] == 0 or c[2] == 1]
    assert any(c[4] == 0 and c[2] > 1 for c in none) and any(c[2] == 1 and c[0] > 1 for c in none)
    for w, h, levels, coarse, refine in none:
        a, b = W.lattice_frames(w, h)
        zero = F.estimate(a, b, levels, coarse, refine, W.LATTICE_LAMBDA)
        want32 = W.estimate_f32(oracle, a, b, levels, coarse, refine, W.LATTICE_LAMBDA, warps=1)
        assert np.array_equal(want32, oracle.flow_estimate(a, b, levels, coarse, refine, W.LATTICE_LAMBDA))
        for warps in range(W.MAX_WARPS + 1):
            assert np.array_equal(W.estimate(a, b, levels, coarse, refine, W.LATTICE_LAMBDA, warps=warps), zero), (w, h, warps)
            if warps:
                got = W.estimate_f32(oracle, a, b, levels, coarse, refine, W.LATTICE_LAMBDA, warps=warps)
                assert np.array_equal(got.view(np.uint32), want32.view(np.uint32)), (w, h, warps)


def test_lattice_tolerance_still_tells_a_wrong_sampler():
    """warps = 4, every scene case in which a round runs (the 3- and 4-level ones among them): nearest sampling is beyond the
    tolerance.  (The noise cases of a few cells are left out: their flows of tens of pixels clamp every sample to a border texel,
    where nearest and bilinear sampling are the same value.)"""
    held = [c for c in W.LATTICE if c[0] >= 60 and c[1] >= 30 and c[2] > 1 and c[4] > 0]
    assert {c[2] for c in held} >= {2, 3, 4}
    for case in held:
        d = _lattice_figure(case, 4, nearest=True)
        print(f"{W.lattice_id(case)} warps 4, nearest sampling in the witness: {d:.3g} px")
        assert d > W.F32_TOLERANCE, (case, d)
