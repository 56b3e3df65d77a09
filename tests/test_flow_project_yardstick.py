"""The yardstick of the dense-flow warp's projection rounds, checked on the CPU (tests/_flow_project.py): the vectorised float32
restatement is the literal per-pixel loop; rounds 0 and t = 0 are the identity; and on the scenes with a rendered true mid-frame
the rounds buy what DESIGN section 8.1 says they buy."""
import numpy as np
import pytest

import _flow_project as PJ
import _flow_warp64 as W
import oracle


def _flows(h, w, seed):
    rng = np.random.default_rng(seed)
    random = ((rng.random((h, w, 2)) - 0.5) * 24).astype(np.float32)  # +-12 px
    step = np.full((h, w, 2), (-3.25, 1.5), np.float32)  # a motion boundary: a quadrant that moves another way
    step[h // 2:, w // 2:] = (7.5, -2.75)
    outside = np.full((h, w, 2), (3.0 * w + 0.5, -2.0 * h - 0.25), np.float32)  # every vector leaves the frame ...
    outside[::2, 1::2] = (-1e4, 1e4)  # ... some of them by far
    return (("random", random), ("step", step), ("outside", outside))


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 2), (5, 3), (13, 9)])
def test_project_f32_is_the_literal_loop(w, h):
    for name, flow in _flows(h, w, 100 * w + h):
        for t in (0.0, 0.25, 0.5, 1.0):
            for rounds in range(PJ.MAX_PROJECT + 1):
                got = PJ.project_f32(flow, t, rounds)
                assert got.dtype == np.float32 and got.shape == flow.shape
                assert np.array_equal(got, PJ.project_loop(flow, t, rounds)), (w, h, name, t, rounds)
    with pytest.raises(ValueError):
        PJ.project_f32(np.zeros((3, 3, 2), np.float32), 0.5, PJ.MAX_PROJECT + 1)
    with pytest.raises(ValueError):
        PJ.project_f32(np.zeros((3, 3), np.float32), 0.5, 1)


def test_rounds_zero_and_time_zero_are_the_identity():
    for name, flow in _flows(9, 13, 5):
        for t in (0.0, 0.3, 1.0):
            assert np.array_equal(PJ.project_f32(flow, t, 0), flow), name
            assert np.array_equal(PJ.project64(flow, t, 0), flow.astype(np.float64)), name
        for rounds in range(1, PJ.MAX_PROJECT + 1):
            assert np.array_equal(PJ.project_f32(flow, 0.0, rounds), flow), (name, rounds)
            assert np.array_equal(PJ.project64(flow, 0.0, rounds), flow.astype(np.float64)), (name, rounds)
    # a constant flow is its own projection at every time; and a round is not the identity on a boundary
    const = np.full((9, 13, 2), (2.5, -1.25), np.float32)
    assert np.array_equal(PJ.project_f32(const, 0.5, 3), const)
    step = _flows(9, 13, 5)[1][1]
    assert not np.array_equal(PJ.project_f32(step, 0.5, 1), step)


@pytest.fixture(scope="module")
def table():
    return [(row,) + PJ.table_row(oracle.warp_blend, row) for row in W.ROWS]


def test_quality_table(table):
    print("\n" + PJ.format_table([(row, psnr) for row, psnr, _ in table]))
    assert len(table) == 7
    for setting in PJ.SETTINGS:
        for i, (row, p, _) in enumerate(table):
            # (a) two rounds lose on no row
            assert p[setting + (2,)] >= p[setting + (0,)] - 0.05, (setting, row, p)
            # (c) every cell is what was measured (tests/_flow_project.py MEASURED; DESIGN 8.1 quotes it)
            for n in PJ.ROUNDS:
                assert p[setting + (n,)] >= PJ.MEASURED[setting][i][n] - 0.05, (setting, row, n, p[setting + (n,)])
    # (b) three rounds behind the best estimator setting gain at least 0.3 dB on at least 4 of the 7 rows
    gains = [p[2, 5, 3] - p[2, 5, 0] for _, p, _ in table]
    print("warps 2, median 5, rounds 3 - rounds 0 (dB): " + ", ".join(f"{g:+.2f}" for g in gains))
    assert sum(g >= 0.3 for g in gains) >= 4, gains


def test_float32_restatement_is_near_the_witness(table):
    """Printed, and held to a bound that follows from the rule: the vector is a bilinear sample of f at a position whose f32
    evaluation is off by at most an ulp of the coordinate (2^-16 px below 256), so one round moves it by at most that times the
    flow's steepest slope (the largest difference of neighbouring cells), plus the few ulps of the lerp itself; N rounds at most
    N times as much where t |slope| <= 1, which holds for these flows' t = 0.5."""
    worst = 0.0
    for row, _, flows in table:
        for (wn, med), flow in flows.items():
            slope = max(float(np.abs(np.diff(flow, axis=0)).max()), float(np.abs(np.diff(flow, axis=1)).max()))
            for n in range(1, PJ.MAX_PROJECT + 1):
                d = float(np.abs(PJ.project_f32(flow, 0.5, n).astype(np.float64) - PJ.project64(flow, 0.5, n)).max())
                worst = max(worst, d)
                bound = n * (2.0 ** -16 * 2 * slope + 8 * 2.0 ** -24 * float(np.abs(flow).max()))
                assert d <= bound, (row, wn, med, n, d, bound)
    print(f"largest |project_f32 - project64| on the table's flows, rounds 1 .. {PJ.MAX_PROJECT}: {worst:.3g} px")
