"""The integer contract of the YUV 4:2:0 kernels (include/nuscaler_hip.h, "YUV 4:2:0 frames"; restated in tests/_yuv.py) against
the float64 witness of the same taps -- real-valued coefficients, one floor(x + 0.5), one clamp: no byte differs by more than 1 and
at most 1 % of the bytes of a form differ.  The per-pixel forms (luma, the chroma formula on the sums of a flat cell at W = 4 and
W = 8, nearest to-RGBA) run over all 2^24 triples; the filtered forms on seeded random 64 x 48 frames plus flat, striped and
checkerboard frames.

Shares measured with this file (differing bytes / bytes; the worst difference is 1 LSB everywhere; run with -s to see them
all).  Exhaustive, per (matrix, range):
    to-YUV luma            601 limited 0.157 %   601 full 0.189 %   709 limited 0.246 %   709 full 0.111 %
    to-YUV chroma          601 limited 0.173 %   601 full 0.338 %   709 limited 0.099 %   709 full 0.000 %
    to-RGBA nearest        601 limited 0.128 %   601 full 0.061 %   709 limited 0.119 %   709 full 0.030 %
Filtered forms, worst over the frames of this file: to-YUV 0.034 % (709 limited, left), to-RGBA 0.048 % (709 limited, bilinear).
The largest share is 0.338 % (BT.601 full range, to-YUV chroma): a third of the cap.
"""
import numpy as np
import pytest

import _yuv as Y

CAP = 0.01
PAIRS = [(m, r) for m in (Y.BT601, Y.BT709) for r in (Y.LIMITED, Y.FULL)]


def _share(a, b):
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return int(d.max()), float((d != 0).mean())


def _report(name, worst, share):
    print(f"{name}: worst difference {worst} LSB, share {100 * share:.3f} %")
    assert worst <= 1, name
    assert share <= CAP, name


def _triples(first, count):
    """`count` consecutive (a, b, c) byte triples from triple number `first`, [count, 3] uint8."""
    i = np.arange(first, first + count, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8)


@pytest.mark.parametrize("matrix,rng", PAIRS)
def test_to_yuv_per_pixel_forms_over_every_triple(matrix, rng):
    """Frames two pixels wide: every pixel a triple of its own for the luma; every 2 x 2 cell flat in one triple for the chroma, so
    the centre sums are 4 (R, G, B).  (The left siting's 8 (R, G, B) give the same bytes, ((8 x + 8 H) >> 17) == ((4 x + 4 H) >> 16)
    for every integer x, and one chunk below checks that; its unequal taps are the filtered tests'.)"""
    chunk = 1 << 20
    diff = {"luma": [0, 0], "chroma W=4": [0, 0]}
    worst = dict.fromkeys(diff, 0)
    for first in range(0, 1 << 24, chunk):
        t = _triples(first, chunk)
        n_y = chunk  # bytes of the luma plane of the frame below
        frame = t.reshape(chunk // 2, 2, 3)
        a, b = Y.to_yuv(frame, matrix, rng, Y.CENTER), Y.to_yuv(frame, matrix, rng, Y.CENTER, real=True)
        w_, s_ = _share(a[:n_y], b[:n_y])
        worst["luma"], diff["luma"] = max(worst["luma"], w_), [diff["luma"][0] + s_ * n_y, diff["luma"][1] + n_y]
        for q in range(4):  # (the chroma costs four pixels a triple: a quarter of the chunk per pass)
            cells = t[q * (chunk // 4):(q + 1) * (chunk // 4)]
            flat = np.repeat(np.repeat(cells.reshape(-1, 1, 3), 2, axis=0), 2, axis=1)  # [2 n, 2, 3]
            a, b = Y.to_yuv(flat, matrix, rng, Y.CENTER, luma=False), Y.to_yuv(flat, matrix, rng, Y.CENTER, real=True, luma=False)
            w_, s_ = _share(a, b)
            worst["chroma W=4"] = max(worst["chroma W=4"], w_)
            diff["chroma W=4"] = [diff["chroma W=4"][0] + s_ * 2 * len(cells), diff["chroma W=4"][1] + 2 * len(cells)]
            if first == 5 * chunk and q == 0:  # (the frame is two pixels wide: the left siting's outer columns clamp into the cell)
                assert (Y.to_yuv(flat, matrix, rng, Y.LEFT, luma=False) == a).all()
    for name in diff:
        _report(f"to-YUV {name} matrix {matrix} range {rng}", worst[name], diff[name][0] / diff[name][1])


@pytest.mark.parametrize("matrix,rng", PAIRS)
def test_nearest_to_rgba_over_every_triple(matrix, rng):
    """Frames two pixels wide: a cell's four luma bytes are four different Y under one (U, V)."""
    cells = 1 << 18
    bad = total = worst = 0
    for first in range(0, 1 << 22, cells):
        i = np.arange(first, first + cells, dtype=np.uint32)  # cell number: U = i >> 14, V = (i >> 6) & 255, Y = 4 (i & 63) + 0 .. 3
        yp = (4 * (i & 63)[:, None] + np.arange(4)[None, :]).astype(np.uint8).reshape(-1)
        frame = np.concatenate([yp, ((i >> 14) & 255).astype(np.uint8), ((i >> 6) & 255).astype(np.uint8)])
        a = Y.to_rgb(frame, 2, 2 * cells, matrix, rng, Y.CENTER, Y.NEAREST)
        b = Y.to_rgb(frame, 2, 2 * cells, matrix, rng, Y.CENTER, Y.NEAREST, real=True)
        w_, s_ = _share(a, b)
        worst, bad, total = max(worst, w_), bad + s_ * a.size, total + a.size
    assert total == 3 << 24
    _report(f"to-RGBA nearest matrix {matrix} range {rng}", worst, bad / total)


def _frames_rgb():
    rng = np.random.default_rng(20240607)
    out = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in range(4)]
    out += [np.full((48, 64, 3), v, np.uint8) for v in (0, 16, 128, 235, 255)]
    x, y = np.meshgrid(np.arange(64), np.arange(48))
    for mask in (x % 2 == 0, y % 2 == 0, (x + y) % 2 == 0, (x // 2 + y // 2) % 2 == 0, x % 3 == 0):
        for lo, hi in (((0, 0, 0), (255, 255, 255)), ((255, 0, 0), (0, 0, 255)), ((16, 200, 40), (235, 20, 220))):
            out.append(np.where(mask[..., None], np.array(hi, np.uint8), np.array(lo, np.uint8)).astype(np.uint8))
    return out


@pytest.mark.parametrize("siting", (Y.CENTER, Y.LEFT))
@pytest.mark.parametrize("matrix,rng", PAIRS)
def test_filtered_to_yuv_is_within_one_lsb(matrix, rng, siting):
    a = np.concatenate([Y.to_yuv(f, matrix, rng, siting) for f in _frames_rgb()])
    b = np.concatenate([Y.to_yuv(f, matrix, rng, siting, real=True) for f in _frames_rgb()])
    _report(f"to-YUV matrix {matrix} range {rng} siting {siting}", *_share(a, b))


@pytest.mark.parametrize("filt", (Y.NEAREST, Y.BILINEAR))
@pytest.mark.parametrize("siting", (Y.CENTER, Y.LEFT))
@pytest.mark.parametrize("matrix,rng", PAIRS)
def test_filtered_to_rgba_is_within_one_lsb(matrix, rng, siting, filt):
    w, h = 64, 48
    # I420 frames: random bytes, and the images of the RGB frames (so that flat, striped and checkerboard chroma occur)
    gen = np.random.default_rng(77)
    frames = [gen.integers(0, 256, Y.frame_bytes(w, h), dtype=np.uint8) for _ in range(4)]
    frames += [Y.to_yuv(f, matrix, rng, siting) for f in _frames_rgb()]
    a = np.concatenate([Y.to_rgb(f, w, h, matrix, rng, siting, filt).reshape(-1) for f in frames])
    b = np.concatenate([Y.to_rgb(f, w, h, matrix, rng, siting, filt, real=True).reshape(-1) for f in frames])
    _report(f"to-RGBA matrix {matrix} range {rng} siting {siting} filter {filt}", *_share(a, b))


def test_restatement_layout_and_clamps():
    """Odd sizes: the planes' sizes, the clamped taps of the last column and row, and the values that must clamp."""
    assert [Y.frame_bytes(*s) for s in ((1, 1), (2, 2), (3, 5), (1920, 1080))] == [3, 6, 27, 3110400]
    rgb = np.zeros((3, 5, 3), np.uint8)
    rgb[:, 4] = 255  # the last column is its cell's only column: the clamped tap doubles it
    out = Y.to_yuv(rgb, Y.BT601, Y.FULL, Y.CENTER)
    yp, up, vp = Y.split(out, 5, 3)
    assert yp.shape == (3, 5) and up.shape == (2, 3) and (yp[:, 4] == 255).all() and (yp[:, :4] == 0).all()
    assert (up[:, 2] == 128).all() and (vp[:, 2] == 128).all() and (up[:, :2] == 128).all()  # white and black are both grey-less
    for filt in (Y.NEAREST, Y.BILINEAR):
        px = Y.to_rgb(np.full(27, 255, np.uint8), 5, 3, Y.BT709, Y.LIMITED, Y.LEFT, filt)
        assert px.min() >= 0 and (px[..., 0] == 255).all()  # far out of gamut: clamped, not wrapped
        px = Y.to_rgb(np.zeros(27, np.uint8), 5, 3, Y.BT709, Y.LIMITED, Y.LEFT, filt)
        assert (px[..., 0] == 0).all() and (px[..., 2] == 0).all()
