"""The NV12 kernels on the MI355X (nus_k_nv12.hip): both conversions and the repack, byte for byte.  An NV12 result is by
definition the I420 result with the chroma bytes in another place, so the expected bytes are tests/_yuv.py's -- the numpy
restatement of the header's integer contract -- passed through tests/_nv12.py's layout: all 16 (matrix, range, siting, filter)
forms, the sizes at which the launcher changes kernels and the kernels meet their edges, the four RGBA formats, pitched surfaces
(row padding, the gap between the planes and the gaps between frames keep their poison), batches, offset bases, the clamps, the
grid-z split and the host entry points.

Kernel forms (nus_k_nv12.hip: nv12_shape, repack_vec): towards RGBA the aligned kernel needs w % 8 == 0 and the NV12 base, pitch,
uv_offset and stride multiples of 8; towards NV12 w % 16 == 0 and multiples of 16; the repack's 16-byte form w % 16 == 0 and
multiples of 16 on both sides; the RGBA side 16-byte aligned throughout.  Everything else runs one pixel / one cell / one byte
per thread."""
import functools

import numpy as np
import pytest

import _nv12 as N
import _yuv as Y
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

POISON = 0x5C
DEV = "cuda:0"
A = (Y.BT709, Y.LIMITED, Y.CENTER, Y.BILINEAR)
B = (Y.BT601, Y.FULL, Y.LEFT, Y.BILINEAR)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _fmt(nsc, form):
    m, r, s, f = form
    return nsc.yuv.YuvFormat(matrix=m, range=r, siting=s, chroma=f)


def _lay(nsc, pitch, uv_off):
    return nsc.yuv.Nv12Layout(pitch, uv_off) if pitch or uv_off else None


@functools.lru_cache(maxsize=None)
def _inputs(w, h, n=1):
    rgba, yuv = Y.random_frames(1900 + 7 * w + 131 * h, n, w, h)
    rgba.setflags(write=False), yuv.setflags(write=False)
    return rgba, yuv


def _want_rgba(i420, w, h, form, px=0):
    m, r, s, f = form
    return np.stack([Y.pack_rgba(Y.to_rgb(fr, w, h, m, r, s, f), px).reshape(-1) for fr in i420])


def _want_i420(rgba, form, px=0):
    m, r, s, _ = form
    return np.stack([Y.to_yuv(Y.unpack_rgba(fr, px), m, r, s) for fr in rgba])


def _nv12_in(i420, w, h, pitch, uv_off, gap, off):
    """I420 frames [n, bytes] -> (device buffer of the NV12 frames of that layout, frame bytes + gap apart, behind `off` bytes;
    frame bytes).  Everything outside the rows holds 0xEE."""
    fr = [N.interleave(x, w, h, pitch, uv_off, fill=0xEE) for x in i420]
    nb = fr[0].size
    buf = np.full(off + len(fr) * (nb + gap), 0xEE, np.uint8)
    buf[off:].reshape(len(fr), nb + gap)[:, :nb] = np.stack(fr)
    return put(buf, DEV), nb


def _out(n, nbytes, gap, off):
    import torch

    return guarded.full((off + n * (nbytes + gap),), POISON, dtype=torch.uint8, device=DEV)


def _frames_of(d_out, n, nbytes, gap, off):
    got = fetch(d_out)
    assert (got[:off] == POISON).all(), "bytes in front of an offset base were written"
    got = got[off:].reshape(n, nbytes + gap)
    assert (got[:, nbytes:] == POISON).all(), "a gap between output frames was written"
    return got[:, :nbytes]


def _to_rgba(nsc, i420, w, h, form, px=0, pitch=0, uv_off=0, nv_gap=0, rgba_gap=0, nv_off=0, rgba_off=0):
    """I420 frames [n, bytes], handed over as NV12 frames of the layout -> nus_nv12_to_rgba8_device's output [n, w h 4]."""
    i420 = np.ascontiguousarray(i420).reshape(len(i420), -1)
    n, fb = len(i420), w * h * 4
    d_in, nb = _nv12_in(i420, w, h, pitch, uv_off, nv_gap, nv_off)
    assert nb == nsc.yuv.nv12_frame_bytes(w, h, _lay(nsc, pitch, uv_off))
    d_out = _out(n, fb, rgba_gap, rgba_off)
    nsc.yuv.nv12_to_rgba_device(d_in.data_ptr() + nv_off, w, h, d_out.data_ptr() + rgba_off, _fmt(nsc, form), n, nb + nv_gap if nv_gap else 0,
                                fb + rgba_gap if rgba_gap else 0, px, _stream(), _lay(nsc, pitch, uv_off))
    return _frames_of(d_out, n, fb, rgba_gap, rgba_off)


def _to_nv12(nsc, rgba, w, h, form, px=0, pitch=0, uv_off=0, nv_gap=0, rgba_gap=0, nv_off=0, rgba_off=0):
    """RGBA frames [n, ...] -> nus_rgba8_to_nv12_device's output frames WHOLE [n, NV12 frame bytes]: what the call left of the
    poison between the rows and the planes is part of the result."""
    rgba = np.ascontiguousarray(rgba).reshape(len(rgba), -1)
    n, fb = rgba.shape
    nb = nsc.yuv.nv12_frame_bytes(w, h, _lay(nsc, pitch, uv_off))
    buf = np.full(rgba_off + n * (fb + rgba_gap), 0xEE, np.uint8)
    buf[rgba_off:].reshape(n, fb + rgba_gap)[:, :fb] = rgba
    d_in = put(buf, DEV)
    d_out = _out(n, nb, nv_gap, nv_off)
    nsc.yuv.rgba_to_nv12_device(d_in.data_ptr() + rgba_off, w, h, d_out.data_ptr() + nv_off, _fmt(nsc, form), n, fb + rgba_gap if rgba_gap else 0,
                                nb + nv_gap if nv_gap else 0, px, _stream(), _lay(nsc, pitch, uv_off))
    return _frames_of(d_out, n, nb, nv_gap, nv_off)


def _want_nv12(i420, w, h, pitch=0, uv_off=0):
    return np.stack([N.interleave(x, w, h, pitch, uv_off, fill=POISON) for x in i420])


def _both(nsc, w, h, form, n=1, px=0, **kw):
    rgba, yuv = _inputs(w, h, n)
    lay = {k: kw[k] for k in ("pitch", "uv_off") if k in kw}
    np.testing.assert_array_equal(_to_rgba(nsc, yuv, w, h, form, px, **kw), _want_rgba(yuv, w, h, form, px), err_msg=f"to RGBA {w}x{h} {form} px {px} {kw}")
    np.testing.assert_array_equal(_to_nv12(nsc, rgba, w, h, form, px, **kw), _want_nv12(_want_i420(rgba, form, px), w, h, **lay),
                                  err_msg=f"to NV12 {w}x{h} {form} px {px} {kw}")


@pytest.mark.parametrize("form", Y.FORMS)
def test_all_sixteen_forms(nsc, form):
    """34 x 5 and 17 x 3 (scalar kernels: a last odd column and row), 32 x 6 and 48 x 5 (the aligned kernels)."""
    for w, h in ((34, 5), (17, 3), (32, 6), (48, 5)):
        _both(nsc, w, h, form)


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 2), (3, 3), (5, 2), (8, 2), (24, 3), (16, 2), (18, 4), (66, 4), (1026, 3), (1040, 3), (2064, 4)])
def test_sizes_where_the_kernels_change_and_meet_their_edges(nsc, w, h):
    """8 x 2 / 24 x 3 are aligned towards RGBA only; 1026 x 3 is two workgroups of the aligned to-RGBA layout plus 2 (scalar); 1040 x 3
    aligned with an odd height; 2064 x 4 two workgroups of the to-NV12 layout plus a run."""
    _both(nsc, w, h, A)
    _both(nsc, w, h, B)


@pytest.mark.parametrize("px", (0, 1, 2, 3))
def test_rgba_formats(nsc, px):
    for w, h in ((34, 5), (32, 4)):
        _both(nsc, w, h, (Y.BT709, Y.LIMITED, Y.LEFT, Y.BILINEAR), px=px)
        _both(nsc, w, h, (Y.BT601, Y.LIMITED, Y.CENTER, Y.NEAREST), px=px)
    rgba, _ = _inputs(34, 5)  # to-NV12 ignores the fourth byte
    other = rgba.copy()
    other[..., 3] ^= 0xFF
    form = (Y.BT709, Y.FULL, Y.CENTER, Y.NEAREST)
    np.testing.assert_array_equal(_to_nv12(nsc, other, 34, 5, form, px), _to_nv12(nsc, rgba, 34, 5, form, px))


@pytest.mark.parametrize("w,h,pitch,uv_off", [(32, 6, 64, 64 * 8), (32, 6, 64, 0), (32, 6, 34, 0), (34, 5, 40, 0), (32, 6, 64, 64 * 6 + 3), (34, 5, 40, 203),
                                              (17, 3, 18, 0), (17, 3, 31, 100)])
def test_pitched_surfaces(nsc, w, h, pitch, uv_off):
    """32 x 6 with pitch 64 (uv_offset 64 * 8, or behind the rows) stays in the aligned kernels; pitch 34, 34 x 5 with pitch 40, and
    uv_offset pitch * h + 3 go to the scalar ones.  Same bytes as tight, and the row padding and the gap between the planes keep the
    poison (_want_nv12 fills them with it); with three frames 48 bytes apart, the gaps between frames too (_frames_of)."""
    for form in (A, B, (Y.BT601, Y.LIMITED, Y.CENTER, Y.NEAREST)):
        _both(nsc, w, h, form, pitch=pitch, uv_off=uv_off)
    _both(nsc, w, h, A, n=3, pitch=pitch, uv_off=uv_off, nv_gap=48, rgba_gap=48)
    rgba, _ = _inputs(w, h)
    tight = _to_nv12(nsc, rgba, w, h, B)
    pitched = _to_nv12(nsc, rgba, w, h, B, pitch=pitch, uv_off=uv_off)
    np.testing.assert_array_equal(np.stack([N.deinterleave(x, w, h, pitch, uv_off) for x in pitched]), np.stack([N.deinterleave(x, w, h) for x in tight]))


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("gap", (0, 48))
def test_batches_tight_and_padded(nsc, n, gap):
    """5 x 3 frames are 27 bytes: tight strides misalign frames 1 and 2.  16 x 2 and 32 x 4 stay in the aligned kernels with either
    stride (48- and 192-byte frames, a 48-byte gap)."""
    for w, h in ((5, 3), (16, 2), (32, 4)):
        _both(nsc, w, h, A, n=n, nv_gap=gap, rgba_gap=gap)
    _both(nsc, 5, 3, (Y.BT601, Y.FULL, Y.LEFT, Y.NEAREST), n=n, nv_gap=gap, rgba_gap=0)


def test_offset_bases_take_the_scalar_kernels_and_give_the_same_bytes(nsc):
    w, h, n = 32, 6, 2
    rgba, yuv = _inputs(w, h, n)
    for form in (A, B, (Y.BT601, Y.LIMITED, Y.CENTER, Y.NEAREST)):
        aligned = _to_rgba(nsc, yuv, w, h, form)
        np.testing.assert_array_equal(aligned, _want_rgba(yuv, w, h, form))
        for kw in (dict(nv_off=1), dict(nv_off=3), dict(nv_off=4), dict(rgba_off=4), dict(nv_off=4, rgba_off=4)):
            np.testing.assert_array_equal(_to_rgba(nsc, yuv, w, h, form, **kw), aligned, err_msg=f"to RGBA {form} {kw}")
        aligned = _to_nv12(nsc, rgba, w, h, form)
        for kw in (dict(nv_off=1), dict(nv_off=3), dict(nv_off=4), dict(rgba_off=4), dict(nv_off=8, rgba_off=4)):
            np.testing.assert_array_equal(_to_nv12(nsc, rgba, w, h, form, **kw), aligned, err_msg=f"to NV12 {form} {kw}")


@pytest.mark.parametrize("w,h", [(16, 2), (6, 2)])
def test_constant_frames_exercise_every_clamp(nsc, w, h):
    """Flat frames of every (a, b, c) over the code values 0, 16, 128, 235, 255, 125 frames a launch: far out of gamut both ways."""
    v = np.array([0, 16, 128, 235, 255], np.uint8)
    trip = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    yuv = np.stack([np.concatenate([np.full(w * h, a, np.uint8), np.full(cw * ch, b, np.uint8), np.full(cw * ch, c, np.uint8)]) for a, b, c in trip])
    rgba = np.stack([np.broadcast_to(np.array([a, b, c, 9], np.uint8), (h, w, 4)) for a, b, c in trip])
    for form in ((Y.BT601, Y.LIMITED, Y.CENTER, Y.BILINEAR), (Y.BT709, Y.LIMITED, Y.LEFT, Y.NEAREST), (Y.BT709, Y.FULL, Y.LEFT, Y.BILINEAR)):
        want = _want_rgba(yuv, w, h, form)
        assert want.min() == 0 and want.max() == 255
        np.testing.assert_array_equal(_to_rgba(nsc, yuv, w, h, form), want)
        want = _want_i420(rgba, form)
        assert (want.min(), want.max()) == ((0, 255) if form[1] == Y.FULL else (16, 240))  # (limited range ends at its own code values)
        np.testing.assert_array_equal(_to_nv12(nsc, rgba, w, h, form), _want_nv12(want, w, h))


def test_65537_frames_cross_the_grid_z_split(nsc):
    """Tight 1 x 1 frames (3 and 4 bytes).  A 1 x 1 NV12 frame is Y, U, V: byte-identical to the 1 x 1 I420 frame, so each direction
    must give what the I420 entry point gives for the same buffer (tests/test_gpu_yuv.py holds that one to the restatement)."""
    import torch

    n = 65537
    rng = np.random.default_rng(65537)
    yuv = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    rgba = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    fmt = _fmt(nsc, A)
    d_yuv, d_rgba = put(yuv.reshape(-1), DEV), put(rgba.reshape(-1), DEV)
    out = [guarded.full((n * 4,), POISON, dtype=torch.uint8, device=DEV) for _ in range(2)]
    nsc.yuv.nv12_to_rgba_device(d_yuv.data_ptr(), 1, 1, out[0].data_ptr(), fmt, n, stream=_stream())
    nsc.yuv.to_rgba_device(d_yuv.data_ptr(), 1, 1, out[1].data_ptr(), fmt, n, stream=_stream())
    got, want = fetch(out[0]).reshape(n, 4), fetch(out[1]).reshape(n, 4)
    assert (want[:, 3] == 255).all() and len(np.unique(want[:, :3], axis=0)) > 1000
    np.testing.assert_array_equal(got, want)
    out = [guarded.full((n * 3,), POISON, dtype=torch.uint8, device=DEV) for _ in range(2)]
    nsc.yuv.rgba_to_nv12_device(d_rgba.data_ptr(), 1, 1, out[0].data_ptr(), fmt, n, stream=_stream())
    nsc.yuv.to_yuv_device(d_rgba.data_ptr(), 1, 1, out[1].data_ptr(), fmt, n, stream=_stream())
    got, want = fetch(out[0]).reshape(n, 3), fetch(out[1]).reshape(n, 3)
    assert len(np.unique(want, axis=0)) > 1000
    np.testing.assert_array_equal(got, want)


def _repack(nsc, to_nv12, src, w, h, pitch=0, uv_off=0, i_gap=0, nv_gap=0, i_off=0, nv_off=0):
    """to_nv12: tight I420 frames [n, bytes] -> nus_yuv420_to_nv12_device's output frames whole; else NV12 frames of the layout
    [n, frame bytes] -> nus_nv12_to_yuv420_device's I420 frames."""
    src = np.ascontiguousarray(src).reshape(len(src), -1)
    n, sb = src.shape
    ib, nb = Y.frame_bytes(w, h), nsc.yuv.nv12_frame_bytes(w, h, _lay(nsc, pitch, uv_off))
    assert sb == (ib if to_nv12 else nb)
    s_gap, s_off, d_gap, d_off, db = (i_gap, i_off, nv_gap, nv_off, nb) if to_nv12 else (nv_gap, nv_off, i_gap, i_off, ib)
    buf = np.full(s_off + n * (sb + s_gap), 0xEE, np.uint8)
    buf[s_off:].reshape(n, sb + s_gap)[:, :sb] = src
    d_in = put(buf, DEV)
    d_out = _out(n, db, d_gap, d_off)
    if to_nv12:
        nsc.yuv.i420_to_nv12_device(d_in.data_ptr() + s_off, w, h, d_out.data_ptr() + d_off, n, ib + i_gap if i_gap else 0, nb + nv_gap if nv_gap else 0,
                                    _stream(), _lay(nsc, pitch, uv_off))
    else:
        nsc.yuv.nv12_to_i420_device(d_in.data_ptr() + s_off, w, h, d_out.data_ptr() + d_off, n, nb + nv_gap if nv_gap else 0, ib + i_gap if i_gap else 0,
                                    _stream(), _lay(nsc, pitch, uv_off))
    return _frames_of(d_out, n, db, d_gap, d_off)


@pytest.mark.parametrize("w,h,pitch,uv_off", [(32, 6, 0, 0), (48, 5, 0, 0), (32, 6, 64, 64 * 8), (2064, 4, 0, 0), (32, 6, 34, 0), (34, 5, 0, 0), (34, 5, 40, 203),
                                              (17, 3, 0, 0), (17, 3, 18, 0), (5, 2, 0, 0), (1, 1, 0, 0), (1, 1, 2, 7), (2, 1, 0, 0), (1, 2, 0, 0), (16, 2, 16, 0)])
def test_repack_moves_bytes_only(nsc, w, h, pitch, uv_off):
    """i420_to_nv12_device(x) is tests/_nv12.interleave(x) with the poison everywhere else, and nv12_to_i420_device takes it back:
    even and odd sizes, tight and pitched, the 16-byte form (32 x 6, 48 x 5, 2064 x 4: two workgroups and more) and the bytewise
    one, three frames with gaps, and offset bases, which must give the aligned call's bytes."""
    _, x = _inputs(w, h, 3)
    want = _want_nv12(x, w, h, pitch, uv_off)
    kw = dict(pitch=pitch, uv_off=uv_off)
    nv = _repack(nsc, True, x, w, h, **kw)
    np.testing.assert_array_equal(nv, want)
    np.testing.assert_array_equal(_repack(nsc, False, nv, w, h, **kw), x)
    for extra in (dict(i_gap=48, nv_gap=32), dict(i_gap=5, nv_gap=7), dict(i_off=1), dict(nv_off=3), dict(i_off=16, nv_off=4)):
        np.testing.assert_array_equal(_repack(nsc, True, x, w, h, **kw, **extra), want, err_msg=f"to NV12 {extra}")
        np.testing.assert_array_equal(_repack(nsc, False, nv, w, h, **kw, **extra), x, err_msg=f"to I420 {extra}")


def test_repack_and_conversions_agree(nsc):
    """rgba -> NV12 directly is rgba -> I420 -> repack, on the device, for an aligned and a scalar shape."""
    import torch

    for w, h in ((32, 6), (17, 3)):
        rgba, _ = _inputs(w, h, 2)
        direct = _to_nv12(nsc, rgba, w, h, B)
        d_rgba = put(np.ascontiguousarray(rgba).reshape(-1), DEV)
        d_i420 = guarded.full((2 * Y.frame_bytes(w, h),), POISON, dtype=torch.uint8, device=DEV)
        nsc.yuv.to_yuv_device(d_rgba.data_ptr(), w, h, d_i420.data_ptr(), _fmt(nsc, B), 2, stream=_stream())
        np.testing.assert_array_equal(_repack(nsc, True, fetch(d_i420).reshape(2, -1), w, h), direct)


def test_host_entry_points_equal_the_device_ones(nsc):
    for (w, h), form in (((34, 5), (Y.BT709, Y.LIMITED, Y.LEFT, Y.BILINEAR)), ((32, 6), (Y.BT601, Y.FULL, Y.CENTER, Y.NEAREST)), ((1, 1), Y.FORMS[3])):
        rgba, yuv = _inputs(w, h)
        fmt = _fmt(nsc, form)
        nv = N.interleave(yuv[0], w, h)
        for px in (0, 1):
            got = np.frombuffer(nsc.yuv.nv12_to_rgba(nv.tobytes(), w, h, fmt, px), np.uint8)
            np.testing.assert_array_equal(got, _to_rgba(nsc, yuv, w, h, form, px)[0])
            np.testing.assert_array_equal(got, _want_rgba(yuv, w, h, form, px)[0])
            got = np.frombuffer(nsc.yuv.rgba_to_nv12(rgba[0].tobytes(), w, h, fmt, px), np.uint8)
            np.testing.assert_array_equal(got, _to_nv12(nsc, rgba, w, h, form, px)[0])
            np.testing.assert_array_equal(got, N.interleave(_want_i420(rgba, form, px)[0], w, h))
