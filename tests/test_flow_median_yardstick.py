"""The yardstick of the flow estimator's median mode, checked on the CPU (tests/_flow_median.py): the float64 witness with median = 0
is tests/_flow_warp64.py's estimator; on the scenes with a rendered true mid-frame the median buys what DESIGN section 8.1 says it
buys; the float32 restatement stays within the tolerance the GPU tests use, and zero padding or a filter on the final flow only
does not."""
import numpy as np
import pytest

import _flow_median as M
import _flow_warp64 as W
import oracle

WIDE = [r for r in W.ROWS if r[0] >= 192]
SMALL = [r for r in W.ROWS if r[0] < 192]
CROP = (67, 45)  # of ROWS[0]: the small size of tests/test_gpu_flow_median.py


@pytest.fixture(scope="module")
def table():
    return [(row, M.table_row(oracle.warp_blend, row)) for row in W.ROWS]


def test_median_filter_is_the_sliding_window_median():
    rng = np.random.default_rng(11)
    for h, w in ((1, 1), (1, 2), (3, 5), (9, 13)):
        flow = ((rng.random((h, w, 2)) - 0.5) * 24).astype(np.float32)
        for size in M.SIZES:
            r = size // 2
            got = M.median_filter(flow, size)
            assert got.dtype == np.float32
            for y in range(h):
                for x in range(w):
                    ys, xs = np.clip(np.arange(y - r, y + r + 1), 0, h - 1), np.clip(np.arange(x - r, x + r + 1), 0, w - 1)
                    for c in range(2):
                        assert got[y, x, c] == np.median(flow[np.ix_(ys, xs)][..., c])  # (an odd count: the middle element)
    with pytest.raises(ValueError):
        M.median_filter(np.zeros((3, 3, 2)), 4)


def test_median_zero_is_the_warp_witness():
    a, b, _ = W.scene(W.ROWS[4])
    for warps in (0, 1, 2):
        assert np.array_equal(M.estimate(a, b, warps=warps, median=0, **W.PARAMS), W.estimate(a, b, warps=warps, **W.PARAMS))
    a, b = a[:45, :67], b[:45, :67]  # odd sizes at every level
    for warps in (0, 1, 2):
        assert np.array_equal(M.estimate(a, b, 4, 7, 3, 4e-4, warps=warps, median=0), W.estimate(a, b, 4, 7, 3, 4e-4, warps=warps))
        want32 = oracle.flow_estimate(a, b, 4, 7, 3, 4e-4) if warps == 0 else W.estimate_f32(oracle, a, b, 4, 7, 3, 4e-4, warps=warps)
        assert np.array_equal(M.estimate_f32(oracle, a, b, 4, 7, 3, 4e-4, warps=warps, median=0).view(np.uint32), want32.view(np.uint32))
    # a run of zero steps is followed by no median: no refining steps leaves the upsampled (filtered) coarsest flow, no coarse steps
    # leaves the zero flow to the first finer level
    for size in M.SIZES:
        got = M.estimate(a, b, 3, 5, 0, 4e-4, warps=2, median=size)
        assert np.array_equal(got, M.estimate(a, b, 3, 5, 0, 4e-4, warps=0, median=size))
        assert not np.array_equal(got, W.estimate(a, b, 3, 5, 0, 4e-4, warps=2))  # (the coarsest run was filtered)
        assert np.array_equal(M.estimate(a, b, 1, 0, 0, 4e-4, median=size), np.zeros((45, 67, 2)))


def test_quality_table(table):
    print("\n" + M.format_table(table))
    for row, p in table:
        gain = {k: p[k] - p[k[0], 0] for k in p if k[1]}
        if row[0] >= 192:
            assert gain[1, 5] >= 0.3 and gain[2, 5] >= 0.5 and gain[1, 3] >= 0.15, (row, gain)
        else:  # 96 x 64: a 5 x 5 window at the coarsest level (24 x 16) covers a quarter of the 6-cell square
            assert min(gain.values()) >= -0.5, (row, gain)
            assert gain[2, 3] >= 0.3 and gain[2, 5] >= 0.3, (row, gain)
    assert len(WIDE) == 6 and len(SMALL) == 1


def _cases():
    out = [(row, W.scene(row)[:2]) for row in W.ROWS]
    a, b, _ = W.scene(W.ROWS[0])
    out.append((CROP, (a[:CROP[1], :CROP[0]].copy(), b[:CROP[1], :CROP[0]].copy())))
    return out


_worst = {}


@pytest.mark.parametrize("size", M.SIZES)
@pytest.mark.parametrize("warps", [1, 2])
def test_float32_restatement_within_tolerance_and_wrong_variants_beyond(warps, size):
    worst = 0.0
    for name, (a, b) in _cases():
        f32 = M.estimate_f32(oracle, a, b, warps=warps, median=size, **W.PARAMS)
        assert f32.dtype == np.float32
        d = float(np.abs(f32 - M.estimate(a, b, warps=warps, median=size, **W.PARAMS)).max())
        d_zero = float(np.abs(f32 - M.estimate(a, b, warps=warps, median=size, pad="constant", **W.PARAMS)).max())
        d_final = float(np.abs(f32 - M.estimate(a, b, warps=warps, median=size, final_only=True, **W.PARAMS)).max())
        d_off = float(np.abs(f32 - W.estimate(a, b, warps=warps, **W.PARAMS)).max())
        print(f"{name} warps {warps} median {size}: |f32 - f64| = {d:.3g} px; zero padding {d_zero:.3g}; final flow only {d_final:.3g}; "
              f"no median {d_off:.3g}")
        worst = max(worst, d)
        assert d <= M.F32_TOLERANCE, (name, d)
        assert d_zero > M.F32_TOLERANCE and d_final > M.F32_TOLERANCE and d_off > M.F32_TOLERANCE, (name, d_zero, d_final, d_off)
    print(f"warps {warps} median {size}: largest |f32 - f64| = {worst:.3g} px, recorded maximum {M.F32_MEASURED_MAX:.3g}, "
          f"tolerance {M.F32_TOLERANCE:.3g}")
    assert worst <= M.F32_MEASURED_MAX  # the recorded figure is the measured maximum, rounded up
    _worst[warps, size] = worst
    if len(_worst) == 4:  # ... by at most one unit of its second digit
        assert max(_worst.values()) >= 0.9 * M.F32_MEASURED_MAX


def test_median_is_non_expansive():
    """|median(a) - median(b)| <= max |a - b|: why the float32 distance needs no allowance for the filter itself."""
    rng = np.random.default_rng(12)
    a = (rng.random((31, 45, 2)) - 0.5) * 24
    b = a + (rng.random(a.shape) - 0.5) * 1e-3
    for size in M.SIZES:
        assert np.abs(M.median_filter(a, size) - M.median_filter(b, size)).max() <= np.abs(a - b).max()
