"""The planar up-scaler of I420 frames on the MI355X (nus_yuv420_resize[_device], yuv.YuvResizer): every plane against the
oracle's bit-exact resize (EXACT mode, centre siting) and against the float64 witness of tests/_plane_resample64.py (both modes,
both sitings), over the shapes at which the kernels meet their borders and change forms, then the forms and the batches.

Kernel forms (nus_k_yuv_resize.hip: plane_rows_form, per plane class).  The row kernel -- a lane owns 4 adjacent output bytes, a
wave a segment of 256 output columns, a workgroup 4 segments and a block of at least 8 output rows -- needs both widths of the
class to be multiples of 4 and every plane of the class on a dword; everything else runs one output byte per thread.  So, in -> out:
  16x8 -> 32x16      row kernel for luma and chroma; every window is cut by a border; two luma row blocks
  22x10 -> 66x30     x3; luma 22 wide and chroma 11x5 -> 33x15 with V on an odd address: per-sample kernel for both classes
  20x10 -> 60x30     x3; row kernel for luma (20 -> 60) beside the per-sample kernel for chroma (10 -> 30; V at byte 250)
  64x36 -> 96x54     x3/2: windows of up to 7 taps (no up-scale has more: test_yuv_resize_host.py); row kernel for both classes
  262x6 -> 1048x12   x4 by x2; per-sample (262 is no multiple of 4), 17 / 9 workgroups along a row
  264x6 -> 1056x12   the same in the row kernel: luma rows span 5 segments (two workgroups), chroma rows 3, the last one partial
  32x18 -> 64x18 / 32x36 / 32x18   one axis unchanged (a 7-tap window at ratio 1), and the copy
  16x20 -> 32x40     5 luma and 3 chroma row blocks on grid.y
Contents, as five frames of one call: seeded noise, all 0, all 255, alternating 0 / 255 columns and rows (the Lanczos and
Catmull-Rom overshoot must clamp)."""
import numpy as np
import pytest

import _plane_resample64 as P
import _resample64 as R
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

POISON = 0x5C
DEV = "cuda:0"
FILTERS = {"lanczos3": 0, "bicubic": 1, "triangle": 2}
FIRST = ((16, 8, 32, 16), (22, 10, 66, 30), (64, 36, 96, 54))
REST = ((20, 10, 60, 30), (262, 6, 1048, 12), (264, 6, 1056, 12), (32, 18, 64, 18), (32, 18, 32, 36), (32, 18, 32, 18), (16, 20, 32, 40))
_cache = {}


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _nbytes(w, h):
    return w * h * 3 // 2


def _split(frame, w, h):
    cw, ch = w // 2, h // 2
    return frame[:w * h].reshape(h, w), frame[w * h:w * h + cw * ch].reshape(ch, cw), frame[w * h + cw * ch:].reshape(ch, cw)


def _frames(w, h):
    """[5, frame bytes]: noise, 0, 255, alternating columns, alternating rows."""
    key = ("in", w, h)
    if key not in _cache:
        rng = np.random.default_rng(4200 + 7 * w + 131 * h)
        out = np.zeros((5, _nbytes(w, h)), np.uint8)
        out[0] = rng.integers(0, 256, _nbytes(w, h), dtype=np.uint8)
        out[2] = 255
        for k, axis in ((3, 1), (4, 0)):
            for pl in _split(out[k], w, h):
                idx = np.arange(pl.shape[axis]) % 2 * 255
                pl[...] = idx[None, :] if axis == 1 else idx[:, None]
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _witness(oracle_mod, shape, alg, siting):
    """Per frame of _frames the float64 planes (Y, U, V), and the contract's eps per plane class; computed once."""
    key = ("v64", shape, alg, siting)
    if key not in _cache:
        iw, ih, ow, oh = shape
        filt = FILTERS[alg]
        phi = 0.25 if siting == "left" else 0.5
        v = []
        for fr in _frames(iw, ih):
            y, u, c = _split(fr, iw, ih)
            v.append((P.plane_resample64(oracle_mod, y, ow, oh, filt, 0.5), P.plane_resample64(oracle_mod, u, ow // 2, oh // 2, filt, phi),
                      P.plane_resample64(oracle_mod, c, ow // 2, oh // 2, filt, phi)))
        eps = (P.plane_eps(oracle_mod, iw, ih, ow, oh, filt, 0.5), P.plane_eps(oracle_mod, iw // 2, ih // 2, ow // 2, oh // 2, filt, phi))
        _cache[key] = (v, eps)
    return _cache[key]


def _exact(oracle_mod, shape, alg):
    """Per frame of _frames the planes of oracle.resize (each plane replicated into four channels; channel 0 of the result)."""
    key = ("exact", shape, alg)
    if key not in _cache:
        iw, ih, ow, oh = shape
        out = []
        for fr in _frames(iw, ih):
            planes = []
            for pl, (pw, ph) in zip(_split(fr, iw, ih), ((ow, oh), (ow // 2, oh // 2), (ow // 2, oh // 2))):
                img = np.ascontiguousarray(np.repeat(pl[:, :, None], 4, axis=2))
                res = np.asarray(oracle_mod.resize(img, pw, ph, FILTERS[alg])).reshape(ph, pw, 4)
                assert (res[..., 0] == res[..., 3]).all()
                planes.append(res[..., 0])
            out.append(np.concatenate([p.reshape(-1) for p in planes]))
        _cache[key] = np.stack(out)
    return _cache[key]


def _run(nsc, src, shape, alg="lanczos3", siting="center", mode="fma", in_gap=0, out_gap=0, in_off=0, out_off=0):
    """src [n, frame bytes] -> the device entry point's output [n, frame bytes]; the gaps between the output frames and the bytes
    in front of an offset base must still hold the poison."""
    import torch

    iw, ih, ow, oh = shape
    src = np.ascontiguousarray(src).reshape(len(src), -1)
    n, in_b = src.shape
    out_b = _nbytes(ow, oh)
    assert in_b == _nbytes(iw, ih)
    buf = np.full(in_off + n * (in_b + in_gap), 0xEE, np.uint8)
    buf[in_off:].reshape(n, in_b + in_gap)[:, :in_b] = src
    d_in = put(buf, DEV)
    d_out = guarded.full((out_off + n * (out_b + out_gap),), POISON, dtype=torch.uint8, device=DEV)
    r = nsc.yuv.YuvResizer(iw, ih, ow, oh, alg, siting, mode)
    r.resize_device(d_in.data_ptr() + in_off, d_out.data_ptr() + out_off, n, in_b + in_gap if in_gap else 0, out_b + out_gap if out_gap else 0,
                    _stream())
    got = fetch(d_out)
    assert (got[:out_off] == POISON).all()
    got = got[out_off:].reshape(n, out_b + out_gap)
    assert (got[:, out_b:] == POISON).all(), "a gap between output frames was written"
    return got[:, :out_b]


def _check(nsc, oracle_mod, shape, alg, siting, mode):
    iw, ih, ow, oh = shape
    got = _run(nsc, _frames(iw, ih), shape, alg, siting, mode)
    v, eps = _witness(oracle_mod, shape, alg, siting)
    for k in range(len(got)):
        for name, g, want, e in zip("YUV", _split(got[k], ow, oh), v[k], (eps[0], eps[1], eps[1])):
            R.assert_fma_contract(g[..., None], want[..., None], e, f"{shape} {alg} {siting} {mode} frame {k} plane {name}")
    if mode == "exact" and siting == "center":
        np.testing.assert_array_equal(got, _exact(oracle_mod, shape, alg), err_msg=f"{shape} {alg} exact centre")
    np.testing.assert_array_equal(got[1], 0)
    np.testing.assert_array_equal(got[2], 255)
    return got


@pytest.mark.parametrize("mode", ("fma", "exact"))
@pytest.mark.parametrize("siting", ("center", "left"))
@pytest.mark.parametrize("alg", tuple(FILTERS))
@pytest.mark.parametrize("shape", FIRST)
def test_every_filter_mode_and_siting(nsc, oracle_mod, shape, alg, siting, mode):
    _check(nsc, oracle_mod, shape, alg, siting, mode)


@pytest.mark.parametrize("mode", ("fma", "exact"))
@pytest.mark.parametrize("siting", ("center", "left"))
@pytest.mark.parametrize("shape", REST)
def test_lanczos_over_the_other_shapes(nsc, oracle_mod, shape, siting, mode):
    got = _check(nsc, oracle_mod, shape, "lanczos3", siting, mode)
    if shape[:2] == shape[2:]:
        np.testing.assert_array_equal(got, _frames(*shape[:2]))  # equal sizes: a copy


def test_the_stripes_overshoot_and_the_sitings_differ(nsc, oracle_mod):
    """The witness of the striped frames leaves 0 .. 255 on both sides (so the clamp is exercised), and left siting moves chroma."""
    shape = (64, 36, 96, 54)
    v, _ = _witness(oracle_mod, shape, "lanczos3", "center")
    assert min(p.min() for p in v[3]) < -1 and max(p.max() for p in v[3]) > 256
    assert min(p.min() for p in v[4]) < -1 and max(p.max() for p in v[4]) > 256
    a = _run(nsc, _frames(64, 36)[:1], shape, siting="center")[0]
    b = _run(nsc, _frames(64, 36)[:1], shape, siting="left")[0]
    ya, ua, va = _split(a, 96, 54)
    yb, ub, vb = _split(b, 96, 54)
    np.testing.assert_array_equal(ya, yb)
    assert (ua != ub).mean() > 0.5 and (va != vb).mean() > 0.5


@pytest.mark.parametrize("mode", ("fma", "exact"))
@pytest.mark.parametrize("shape", ((16, 8, 32, 16), (64, 36, 96, 54), (264, 6, 1056, 12), (20, 10, 60, 30), (32, 18, 32, 18)))
def test_offset_bases_take_the_per_sample_form_and_give_the_same_bytes(nsc, shape, mode):
    src = _frames(*shape[:2])[:2]
    for siting in ("center", "left"):
        aligned = _run(nsc, src, shape, siting=siting, mode=mode)
        for kw in (dict(in_off=1), dict(out_off=1), dict(in_off=1, out_off=1), dict(in_off=3, out_off=2)):
            np.testing.assert_array_equal(_run(nsc, src, shape, siting=siting, mode=mode, **kw), aligned, err_msg=f"{shape} {siting} {kw}")


@pytest.mark.parametrize("shape", ((16, 8, 32, 16), (22, 10, 66, 30), (64, 36, 96, 54), (32, 18, 32, 18)))
def test_three_frames_with_padded_strides_equal_three_calls(nsc, shape):
    """in: frame + 24, out: frame + 40 (both keep the row kernel's dword alignment), then in: frame + 5, out: frame + 7 (odd
    strides: the whole launch goes to the per-sample form); the gaps keep their poison (_run)."""
    src = _frames(*shape[:2])[[0, 3, 4]]
    for alg, siting in (("lanczos3", "left"), ("bicubic", "center")):
        single = np.concatenate([_run(nsc, src[k:k + 1], shape, alg, siting) for k in range(3)])
        np.testing.assert_array_equal(_run(nsc, src, shape, alg, siting), single)
        np.testing.assert_array_equal(_run(nsc, src, shape, alg, siting, in_gap=24, out_gap=40), single)
        np.testing.assert_array_equal(_run(nsc, src, shape, alg, siting, in_gap=5, out_gap=7), single)


def test_host_entry_point_equals_the_device_one(nsc):
    for shape, alg, siting, mode in (((16, 8, 32, 16), "lanczos3", "left", "fma"), ((22, 10, 66, 30), "triangle", "center", "exact"),
                                     ((64, 36, 96, 54), "bicubic", "left", "exact"), ((32, 18, 32, 18), "lanczos3", "center", "fma")):
        src = _frames(*shape[:2])
        r = nsc.yuv.YuvResizer(*shape, alg, siting, mode)
        dev = _run(nsc, src[[0, 3]], shape, alg, siting, mode)
        for k, j in ((0, 0), (3, 1)):
            got = np.frombuffer(r.resize(src[k].tobytes()), np.uint8)
            np.testing.assert_array_equal(got, dev[j], err_msg=f"{shape} {alg} frame {k}")
