"""The numpy yardstick of the scene-cut detector (tests/_scenecut.py) against a literal per-pixel loop over small frames, and
the figures the issue quotes for the decision cases (so the GPU test's margins rest on checked numbers).  CPU only."""
import numpy as np
import pytest

import _scenecut as sc


def _loop_measures(a, b, fmt):
    h, w = a.shape[:2]
    sad = 0
    ha, hb = [0] * 32, [0] * 32
    for y in range(h):
        for x in range(w):
            pa, pb = [int(v) for v in a[y, x]], [int(v) for v in b[y, x]]
            sad += abs(pa[0] - pb[0]) + abs(pa[1] - pb[1]) + abs(pa[2] - pb[2])
            for p, hist in ((pa, ha), (pb, hb)):
                r, g, bl = (p[2], p[1], p[0]) if fmt in (sc.BGRA, sc.BGRX) else (p[0], p[1], p[2])
                lum = (77 * r + 150 * g + 29 * bl + 128) >> 8
                assert 0 <= lum <= 255
                hist[lum >> 3] += 1
    return sad, sum(abs(p - q) for p, q in zip(ha, hb))


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (17, 9), (32, 16)])
@pytest.mark.parametrize("fmt", [sc.RGBA, sc.BGRA, sc.RGBX, sc.BGRX])
def test_measures_equal_the_pixel_loop(w, h, fmt):
    rng = np.random.default_rng(100 * w + h + fmt)
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    b = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    assert sc.measures(a, b, fmt) == _loop_measures(a, b, fmt)
    assert sc.measures(a, a, fmt) == (0, 0)


def test_extremes():
    a = np.zeros((5, 4, 4), np.uint8)
    b = np.full((5, 4, 4), 255, np.uint8)
    assert sc.measures(a, b) == (3 * 255 * 20, 2 * 20)  # white is Y = 255 exactly: the weights sum to 256
    assert sc.luma_hist(b)[31] == 20


def test_bgra_gives_the_numbers_of_the_swizzled_rgba():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (9, 17, 4), dtype=np.uint8)
    b = rng.integers(0, 256, (9, 17, 4), dtype=np.uint8)
    assert sc.measures(a[..., [2, 1, 0, 3]], b[..., [2, 1, 0, 3]], sc.BGRA) == sc.measures(a, b, sc.RGBA)
    red = np.zeros((4, 4, 4), np.uint8)
    red[..., 0] = 255
    blue = np.zeros((4, 4, 4), np.uint8)
    blue[..., 2] = 255
    assert sc.measures(red, blue, sc.RGBA)[1] == 32 and sc.measures(red, blue, sc.RGBA) == sc.measures(blue, red, sc.BGRA)


def test_decision_is_the_integer_rule():
    w, h = 10, 10
    assert sc.is_cut(20 * 300, 80, w, h) and not sc.is_cut(20 * 300 - 1, 80, w, h) and not sc.is_cut(20 * 300, 79, w, h)
    assert sc.is_cut(0, 0, w, h, 0, 0)
    assert not sc.is_cut(255 * 300 - 1, 200, w, h, 255, 1000) and sc.is_cut(255 * 300, 200, w, h, 255, 1000)


def test_copy_and_apply():
    rng = np.random.default_rng(6)
    a = rng.integers(0, 256, (2, 3, 5, 4), dtype=np.uint8)
    b = rng.integers(0, 256, (2, 3, 5, 4), dtype=np.uint8)
    assert np.array_equal(sc.copy_of(a[0], sc.BGRX)[..., :3], a[0][..., [2, 1, 0]]) and (sc.copy_of(a[0], sc.BGRX)[..., 3] == 255).all()
    times = [0.0, 0.25, 0.5, 1.0]
    out = np.full((2, 4, 3, 5, 4), 0xA7, np.uint8)
    sc.apply_cuts(a, b, [0, 1], times, out)
    assert (out[0] == 0xA7).all()
    assert np.array_equal(out[1, 0], a[1]) and np.array_equal(out[1, 1], a[1])
    assert np.array_equal(out[1, 2], b[1]) and np.array_equal(out[1, 3], b[1])


def test_the_decision_cases_have_the_margins_the_contract_quotes():
    """MAD / histogram permille at 320 x 180 of the contents tests/test_gpu_scenecut.py decides on."""
    from _scenecut_content import decision_cases

    for name, a, b, want_cut, mad_range, hist_range in decision_cases(320, 180):
        sad, hist = sc.measures(a, b)
        mad, permille = sc.mad_and_permille(sad, hist, 320, 180)
        assert mad_range[0] <= mad <= mad_range[1], (name, mad)
        assert hist_range[0] <= permille <= hist_range[1], (name, permille)
        assert sc.is_cut(sad, hist, 320, 180) == want_cut, name
