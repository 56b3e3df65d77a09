"""The planar up-scaler on tight NV12 frames on the MI355X (nus_nv12_resize[_device], YuvResizer.resize_nv12[_device]).  The
contract is equality: the output is nus_yuv420_resize_device's output on the de-interleaved input, interleaved again, bit for bit
in both modes.  On top of that every de-interleaved plane is held to what tests/test_gpu_yuv_resize.py holds the I420 planes to:
oracle.resize (EXACT mode, centre siting) and the float64 witness of tests/_plane_resample64.py with the unchanged eps_rule.

Chroma forms (nus_k_nv12_resize.hip: pair_rows_form).  The pair row kernel -- a lane owns 4 adjacent output bytes (two U,V pairs),
a wave a segment of 128 output pairs -- needs both luma widths to be multiples of 4 and every base and stride on a dword;
everything else runs one output byte per thread.  In -> out:
  8x8 -> 16x16       row form; every window is cut by a border
  16x20 -> 32x40     row form; three chroma row blocks on grid.y
  12x8 -> 16x12      row form at ratio 4/3
  8x8 -> 8x16        row form, x unchanged (the 7-tap windows and the 8-wide union of ratio 1)
  504x4 -> 512x8     row form; a chroma row is one full segment (128 pairs) whose input footprint exceeds 256 bytes: two V sweeps
  22x6 -> 26x10      per-sample form for chroma (26 % 4 != 0)
Contents, as five frames of one call: seeded noise, all 0, all 255, alternating 0 / 255 columns and rows."""
import numpy as np
import pytest

import _nv12 as N
import _resample64 as R
import test_gpu_yuv_resize as T
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

POISON = 0x5C
DEV = "cuda:0"
SHAPES = (((8, 8, 16, 16), True), ((16, 20, 32, 40), True), ((12, 8, 16, 12), True), ((8, 8, 8, 16), True), ((504, 4, 512, 8), True), ((22, 6, 26, 10), False))


def _inter(frames, w, h):
    """[n, I420 bytes] -> [n, tight NV12 bytes], even sizes, all frames at once (tests/_nv12.interleave frame by frame is the rule;
    test_the_batch_interleave_is_the_yardsticks holds this to it)."""
    frames = np.asarray(frames)
    n, c = len(frames), (w // 2) * (h // 2)
    out = np.empty_like(frames)
    out[:, :w * h] = frames[:, :w * h]
    out[:, w * h:] = np.stack([frames[:, w * h:w * h + c], frames[:, w * h + c:]], axis=-1).reshape(n, 2 * c)
    return out


def _deinter(frames, w, h):
    frames = np.asarray(frames)
    n, c = len(frames), (w // 2) * (h // 2)
    uv = frames[:, w * h:].reshape(n, c, 2)
    return np.concatenate([frames[:, :w * h], uv[:, :, 0], uv[:, :, 1]], axis=1)


def test_the_batch_interleave_is_the_yardsticks():
    x = T._frames(12, 8)
    np.testing.assert_array_equal(_inter(x, 12, 8), np.stack([N.interleave(f, 12, 8) for f in x]))
    np.testing.assert_array_equal(_deinter(_inter(x, 12, 8), 12, 8), x)
    np.testing.assert_array_equal(_deinter(_inter(x, 12, 8), 12, 8), np.stack([N.deinterleave(f, 12, 8) for f in _inter(x, 12, 8)]))


def _run(nsc, i420, shape, alg="lanczos3", siting="center", mode="fma", in_gap=0, out_gap=0, in_off=0, out_off=0):
    """I420 frames [n, bytes], handed over as tight NV12 frames -> nus_nv12_resize_device's NV12 output [n, bytes]; the gaps between
    the output frames and the bytes in front of an offset base must still hold the poison."""
    import torch

    iw, ih, ow, oh = shape
    src = _inter(np.ascontiguousarray(i420).reshape(len(i420), -1), iw, ih)
    n, in_b = src.shape
    out_b = T._nbytes(ow, oh)
    assert in_b == T._nbytes(iw, ih)
    buf = np.full(in_off + n * (in_b + in_gap), 0xEE, np.uint8)
    buf[in_off:].reshape(n, in_b + in_gap)[:, :in_b] = src
    d_in = put(buf, DEV)
    d_out = guarded.full((out_off + n * (out_b + out_gap),), POISON, dtype=torch.uint8, device=DEV)
    r = nsc.yuv.YuvResizer(iw, ih, ow, oh, alg, siting, mode)
    r.resize_nv12_device(d_in.data_ptr() + in_off, d_out.data_ptr() + out_off, n, in_b + in_gap if in_gap else 0, out_b + out_gap if out_gap else 0,
                         T._stream())
    got = fetch(d_out)
    assert (got[:out_off] == POISON).all()
    got = got[out_off:].reshape(n, out_b + out_gap)
    assert (got[:, out_b:] == POISON).all(), "a gap between output frames was written"
    return got[:, :out_b]


@pytest.mark.parametrize("mode", ("fma", "exact"))
@pytest.mark.parametrize("siting", ("center", "left"))
@pytest.mark.parametrize("alg", tuple(T.FILTERS))
@pytest.mark.parametrize("shape", [s for s, _ in SHAPES])
def test_every_shape_filter_mode_and_siting(nsc, oracle_mod, shape, alg, siting, mode):
    iw, ih, ow, oh = shape
    src = T._frames(iw, ih)
    got = _run(nsc, src, shape, alg, siting, mode)
    planar = T._run(nsc, src, shape, alg, siting, mode)  # nus_yuv420_resize_device on the de-interleaved input
    np.testing.assert_array_equal(got, _inter(planar, ow, oh), err_msg=f"{shape} {alg} {siting} {mode}: not the I420 output rearranged")
    de = _deinter(got, ow, oh)
    v, eps = T._witness(oracle_mod, shape, alg, siting)
    for k in range(len(de)):
        for name, g, want, e in zip("YUV", T._split(de[k], ow, oh), v[k], (eps[0], eps[1], eps[1])):
            R.assert_fma_contract(g[..., None], want[..., None], e, f"{shape} {alg} {siting} {mode} frame {k} plane {name}")
    if mode == "exact" and siting == "center":
        np.testing.assert_array_equal(de, T._exact(oracle_mod, shape, alg), err_msg=f"{shape} {alg} exact centre")
    np.testing.assert_array_equal(got[1], 0)
    np.testing.assert_array_equal(got[2], 255)
    assert len(np.unique(got[3])) > 1 and len(np.unique(got[4])) > 1


@pytest.mark.parametrize("mode", ("fma", "exact"))
@pytest.mark.parametrize("shape", ((8, 8, 16, 16), (12, 8, 16, 12), (504, 4, 512, 8), (22, 6, 26, 10), (16, 20, 16, 20)))
def test_offset_bases_take_the_per_sample_form_and_give_the_same_bytes(nsc, shape, mode):
    src = T._frames(*shape[:2])[[0, 3]]
    for siting in ("center", "left"):
        aligned = _run(nsc, src, shape, siting=siting, mode=mode)
        for kw in (dict(in_off=1), dict(out_off=1), dict(in_off=2, out_off=2), dict(in_off=3, out_off=1)):
            np.testing.assert_array_equal(_run(nsc, src, shape, siting=siting, mode=mode, **kw), aligned, err_msg=f"{shape} {siting} {kw}")


@pytest.mark.parametrize("shape", ((8, 8, 16, 16), (22, 6, 26, 10), (12, 8, 16, 12), (16, 20, 16, 20)))
def test_three_frames_with_padded_strides_equal_three_calls(nsc, shape):
    """in: frame + 24, out: frame + 40 (both keep the row kernel's dword alignment), then in: frame + 5, out: frame + 7 (odd
    strides: the whole launch goes to the per-sample form); the gaps keep their poison (_run)."""
    src = T._frames(*shape[:2])[[0, 3, 4]]
    for alg, siting in (("lanczos3", "left"), ("bicubic", "center")):
        single = np.concatenate([_run(nsc, src[k:k + 1], shape, alg, siting) for k in range(3)])
        np.testing.assert_array_equal(_run(nsc, src, shape, alg, siting), single)
        np.testing.assert_array_equal(_run(nsc, src, shape, alg, siting, in_gap=24, out_gap=40), single)
        np.testing.assert_array_equal(_run(nsc, src, shape, alg, siting, in_gap=5, out_gap=7), single)


def test_equal_sizes_copy(nsc):
    src = T._frames(16, 20)
    np.testing.assert_array_equal(_run(nsc, src, (16, 20, 16, 20)), _inter(src, 16, 20))


def test_host_entry_point_equals_the_device_one(nsc):
    for shape, alg, siting, mode in (((8, 8, 16, 16), "lanczos3", "left", "fma"), ((22, 6, 26, 10), "triangle", "center", "exact"),
                                     ((12, 8, 16, 12), "bicubic", "left", "exact"), ((16, 20, 16, 20), "lanczos3", "center", "fma")):
        src = T._frames(*shape[:2])
        r = nsc.yuv.YuvResizer(*shape, alg, siting, mode)
        dev = _run(nsc, src[[0, 3]], shape, alg, siting, mode)
        for k, j in ((0, 0), (3, 1)):
            got = np.frombuffer(r.resize_nv12(N.interleave(src[k], *shape[:2]).tobytes()), np.uint8)
            np.testing.assert_array_equal(got, dev[j], err_msg=f"{shape} {alg} frame {k}")


@pytest.mark.parametrize("mode", ("fma", "exact"))
def test_65537_frames_cross_the_grid_z_split_of_the_chroma_launch(nsc, mode):
    """4 x 4 -> 8 x 8, tight (24 and 96 bytes: the pair row kernel): frame 65535 is the first of the second chroma launch.  Equal to
    the I420 entry point's output for the de-interleaved batch, rearranged."""
    n, shape = 65537, (4, 4, 8, 8)
    src = np.random.default_rng(8812).integers(0, 256, (n, 24), dtype=np.uint8)
    src[65534:65537, 16:] = [[0] * 4 + [255] * 4, [255] * 4 + [0] * 4, [255] * 8]  # flat U and V planes around the split: a channel mix-up shows
    got = _run(nsc, src, shape, mode=mode)
    want = _inter(T._run(nsc, src, shape, mode=mode), 8, 8)
    np.testing.assert_array_equal(got[65530:], want[65530:])
    np.testing.assert_array_equal(got, want)
    assert (got[65534, 64::2] == 0).all() and (got[65534, 65::2] == 255).all() and (got[65536, 64:] == 255).all()
