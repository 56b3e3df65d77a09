"""The YUV 4:2:0 kernels on the MI355X: both directions byte for byte against the numpy restatement of the header's integer
contract (tests/_yuv.py) -- all 16 (matrix, range, siting, filter) forms, the sizes at which the launcher changes kernels and the
kernels meet their edges, the four RGBA formats, batches with tight and padded strides (gaps stay poisoned), bases that push an
aligned shape to the scalar kernels, the clamps, the grid-z split and the host entry points.

Kernel forms (nus_k_yuv.hip: yuv_shape): towards RGBA the aligned kernel needs w % 8 == 0, towards YUV w % 16 == 0, both 16-byte
aligned bases and strides; everything else runs one pixel / one chroma cell per thread.  A workgroup of the aligned kernels spans
512 / 1024 pixels of a row pair, one of the scalar kernels 64 pixels / 64 cells."""
import functools

import numpy as np
import pytest

import _yuv as Y
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

POISON = 0x5C
DEV = "cuda:0"


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _fmt(nsc, form):
    m, r, s, f = form
    return nsc.yuv.YuvFormat(matrix=m, range=r, siting=s, chroma=f)


@functools.lru_cache(maxsize=None)
def _inputs(w, h, n=1):
    rgba, yuv = Y.random_frames(900 + 7 * w + 131 * h, n, w, h)
    rgba.setflags(write=False), yuv.setflags(write=False)
    return rgba, yuv


def _want_rgba(yuv, w, h, form, px=0):
    m, r, s, f = form
    return np.stack([Y.pack_rgba(Y.to_rgb(fr, w, h, m, r, s, f), px).reshape(-1) for fr in yuv])


def _want_yuv(rgba, form, px=0):
    m, r, s, _ = form
    return np.stack([Y.to_yuv(Y.unpack_rgba(fr, px), m, r, s) for fr in rgba])


def _run(nsc, to_rgba, src, w, h, form, px=0, in_gap=0, out_gap=0, in_off=0, out_off=0):
    """src [n, frame bytes] uint8 -> the device entry point's output [n, frame bytes]; checks that the gaps between the output
    frames and the bytes in front of an offset base still hold the poison."""
    import torch

    src = np.ascontiguousarray(src).reshape(len(src), -1)
    n, in_bytes = src.shape
    yb, fb = Y.frame_bytes(w, h), w * h * 4
    out_bytes = fb if to_rgba else yb
    assert in_bytes == (yb if to_rgba else fb)
    buf = np.full(in_off + n * (in_bytes + in_gap), 0xEE, np.uint8)
    buf[in_off:].reshape(n, in_bytes + in_gap)[:, :in_bytes] = src
    d_in = put(buf, DEV)
    d_out = guarded.full((out_off + n * (out_bytes + out_gap),), POISON, dtype=torch.uint8, device=DEV)
    fmt = _fmt(nsc, form)
    tight_in, tight_out = in_gap == 0, out_gap == 0
    if to_rgba:
        nsc.yuv.to_rgba_device(d_in.data_ptr() + in_off, w, h, d_out.data_ptr() + out_off, fmt, n, 0 if tight_in else in_bytes + in_gap,
                               0 if tight_out else out_bytes + out_gap, px, _stream())
    else:
        nsc.yuv.to_yuv_device(d_in.data_ptr() + in_off, w, h, d_out.data_ptr() + out_off, fmt, n, 0 if tight_in else in_bytes + in_gap,
                              0 if tight_out else out_bytes + out_gap, px, _stream())
    got = fetch(d_out)
    assert (got[:out_off] == POISON).all()
    got = got[out_off:].reshape(n, out_bytes + out_gap)
    assert (got[:, out_bytes:] == POISON).all(), "a gap between output frames was written"
    return got[:, :out_bytes]


def _both(nsc, w, h, form, n=1, px=0, **kw):
    rgba, yuv = _inputs(w, h, n)
    got = _run(nsc, True, yuv, w, h, form, px, **kw)
    np.testing.assert_array_equal(got, _want_rgba(yuv, w, h, form, px), err_msg=f"to RGBA {w}x{h} {form} px {px} {kw}")
    got = _run(nsc, False, rgba, w, h, form, px, **kw)
    np.testing.assert_array_equal(got, _want_yuv(rgba, form, px), err_msg=f"to YUV {w}x{h} {form} px {px} {kw}")


@pytest.mark.parametrize("form", Y.FORMS)
def test_all_sixteen_forms(nsc, form):
    """34 x 5 and 17 x 3 (scalar kernels: odd sizes, a last column and row of their own), 32 x 6 and 48 x 5 (the aligned kernels)."""
    for w, h in ((34, 5), (17, 3), (32, 6), (48, 5)):
        _both(nsc, w, h, form)


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 2), (3, 3), (5, 2), (16, 2), (18, 4), (66, 4), (130, 7), (8, 2), (24, 3), (1026, 3), (1040, 3), (2064, 4)])
def test_sizes_where_the_kernels_change_and_meet_their_edges(nsc, w, h):
    """The issue's sizes, then 8 x 2 / 24 x 3 (aligned towards RGBA, scalar towards YUV), 1026 x 3 (two workgroups of the aligned
    to-RGBA layout plus 2: the scalar kernels over seventeen workgroups), 1040 x 3 (aligned, odd height, three / two workgroups) and
    2064 x 4 (two workgroups of the aligned to-YUV layout plus a run)."""
    _both(nsc, w, h, (Y.BT709, Y.LIMITED, Y.CENTER, Y.BILINEAR))
    _both(nsc, w, h, (Y.BT601, Y.FULL, Y.LEFT, Y.BILINEAR))


@pytest.mark.parametrize("px", (0, 1, 2, 3))
def test_rgba_formats(nsc, px):
    for w, h in ((34, 5), (32, 4)):
        _both(nsc, w, h, (Y.BT709, Y.LIMITED, Y.LEFT, Y.BILINEAR), px=px)
        _both(nsc, w, h, (Y.BT601, Y.LIMITED, Y.CENTER, Y.NEAREST), px=px)
    # to-YUV ignores the fourth byte
    rgba, _ = _inputs(34, 5)
    other = rgba.copy()
    other[..., 3] ^= 0xFF
    form = (Y.BT709, Y.FULL, Y.CENTER, Y.NEAREST)
    np.testing.assert_array_equal(_run(nsc, False, other, 34, 5, form, px), _run(nsc, False, rgba, 34, 5, form, px))


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("gap", (0, 48))
def test_batches_tight_and_padded(nsc, n, gap):
    """5 x 3 frames are 27 bytes: tight strides misalign frames 1 and 2.  16 x 2 and 32 x 4 stay in the aligned kernels with either
    stride (48- and 192-byte frames, a 48-byte gap)."""
    form = (Y.BT709, Y.LIMITED, Y.CENTER, Y.BILINEAR)
    for w, h in ((5, 3), (16, 2), (32, 4)):
        _both(nsc, w, h, form, n=n, in_gap=gap, out_gap=gap)
    _both(nsc, 5, 3, (Y.BT601, Y.FULL, Y.LEFT, Y.NEAREST), n=n, in_gap=gap, out_gap=0)


def test_offset_bases_take_the_scalar_kernels_and_give_the_same_bytes(nsc):
    w, h, n = 32, 6, 2
    rgba, yuv = _inputs(w, h, n)
    for form in ((Y.BT709, Y.LIMITED, Y.CENTER, Y.BILINEAR), (Y.BT601, Y.FULL, Y.LEFT, Y.BILINEAR), (Y.BT601, Y.LIMITED, Y.CENTER, Y.NEAREST)):
        for to_rgba, src in ((True, yuv), (False, rgba)):
            aligned = _run(nsc, to_rgba, src, w, h, form)
            for kw in (dict(in_off=4), dict(out_off=4), dict(in_off=4, out_off=4)):
                np.testing.assert_array_equal(_run(nsc, to_rgba, src, w, h, form, **kw), aligned, err_msg=f"{form} {to_rgba} {kw}")
            if to_rgba:  # the YUV side has no alignment rule at all
                np.testing.assert_array_equal(_run(nsc, True, src, w, h, form, in_off=1), aligned)
            else:
                np.testing.assert_array_equal(_run(nsc, False, src, w, h, form, out_off=3), aligned)
    np.testing.assert_array_equal(_run(nsc, True, yuv, w, h, (Y.BT709, Y.LIMITED, Y.CENTER, Y.BILINEAR)),
                                  _want_rgba(yuv, w, h, (Y.BT709, Y.LIMITED, Y.CENTER, Y.BILINEAR)))


@pytest.mark.parametrize("w,h", [(16, 2), (6, 2)])
def test_constant_frames_exercise_every_clamp(nsc, w, h):
    """Flat frames of every (a, b, c) over the code values 0, 16, 128, 235, 255, 125 frames a launch: far out of gamut both ways."""
    v = np.array([0, 16, 128, 235, 255], np.uint8)
    trip = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    yuv = np.stack([np.concatenate([np.full(w * h, a, np.uint8), np.full(cw * ch, b, np.uint8), np.full(cw * ch, c, np.uint8)]) for a, b, c in trip])
    rgba = np.stack([np.broadcast_to(np.array([a, b, c, 9], np.uint8), (h, w, 4)) for a, b, c in trip])
    for form in ((Y.BT601, Y.LIMITED, Y.CENTER, Y.BILINEAR), (Y.BT709, Y.LIMITED, Y.LEFT, Y.NEAREST), (Y.BT709, Y.FULL, Y.LEFT, Y.BILINEAR)):
        got = _run(nsc, True, yuv, w, h, form)
        want = _want_rgba(yuv, w, h, form)
        assert want.min() == 0 and want.max() == 255
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(_run(nsc, False, rgba, w, h, form), _want_yuv(rgba, form))


def test_65537_frames_cross_the_grid_z_split(nsc):
    """1 x 1 frames, tight (3 and 4 bytes).  The restatement of all of them at once: frame i as cell i of a frame two pixels wide
    -- a 1 x 1 frame's clamped taps all land on its one pixel, which is a flat cell; its bilinear chroma is 16 times its one
    sample, which gives the nearest filter's bytes ((16 x + 16 H) >> 18 == (x + H) >> 14), so the big frame, whose cells must not
    mix, is converted with that filter."""
    n = 65537
    rng = np.random.default_rng(65537)
    yuv = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    rgba = rng.integers(0, 256, (n, 1, 1, 4), dtype=np.uint8)
    m, r, s, f = form = (Y.BT709, Y.LIMITED, Y.CENTER, Y.BILINEAR)
    cells = np.concatenate([np.repeat(yuv[:, 0], 4), yuv[:, 1], yuv[:, 2]])
    want = Y.pack_rgba(Y.to_rgb(cells, 2, 2 * n, m, r, s, Y.NEAREST))[0::2, 0].reshape(n, 4)
    np.testing.assert_array_equal(_run(nsc, True, yuv, 1, 1, form), want)
    flat = np.repeat(np.repeat(rgba[:, 0, :, :3], 2, axis=0), 2, axis=1)  # [2 n, 2, 3]
    out = Y.to_yuv(flat, m, r, s)
    yp, up, vp = Y.split(out, 2, 2 * n)
    want = np.stack([yp[0::2, 0], up[:, 0], vp[:, 0]], axis=-1)
    np.testing.assert_array_equal(_run(nsc, False, rgba, 1, 1, form), want)


def test_host_entry_points_equal_the_device_ones(nsc):
    for (w, h), form in (((34, 5), (Y.BT709, Y.LIMITED, Y.LEFT, Y.BILINEAR)), ((32, 6), (Y.BT601, Y.FULL, Y.CENTER, Y.NEAREST)), ((1, 1), Y.FORMS[3])):
        rgba, yuv = _inputs(w, h)
        fmt = _fmt(nsc, form)
        for px in (0, 1):
            got = np.frombuffer(nsc.yuv.to_rgba(yuv[0].tobytes(), w, h, fmt, px), np.uint8)
            np.testing.assert_array_equal(got, _run(nsc, True, yuv, w, h, form, px)[0])
            np.testing.assert_array_equal(got, _want_rgba(yuv, w, h, form, px)[0])
            got = np.frombuffer(nsc.yuv.to_yuv(rgba[0].tobytes(), w, h, fmt, px), np.uint8)
            np.testing.assert_array_equal(got, _run(nsc, False, rgba, w, h, form, px)[0])
            np.testing.assert_array_equal(got, _want_yuv(rgba, form, px)[0])
