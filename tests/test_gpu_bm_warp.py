"""nus_bm_warp_device on the MI355X, the kernel alone: per-block vectors made by hand (no search), warped and blended straight from
them.  EXACT mode is byte for byte the oracle's warp + blend of the expanded vectors; FMA mode holds the interpolation path's
contract against it (no byte off by more than 1; at 328 x 200, the shape the cap is defined on, fewer than 0.1 % of the bytes
differing).  Shapes: the tiny form (1 x 1, 1 x 9), an odd single partial block (7 x 5), partial blocks right and bottom at every
block size (33 x 17), several workgroups across and several block rows (200 x 72), and 328 x 200.  With vectors uniform in
[-24, 24] most samples of the small shapes leave the frame: the clamp, the w - 2 / h - 2 corner rule and the block seams all
work.  Every device output lives in a conftest.guarded tensor and comes down through nus_download."""
import functools

import numpy as np
import pytest

import _blockmatch as bmref
from _warp64 import warp_contract
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (7, 5), (33, 17), (200, 72), (328, 200)]
BLOCK_SIZES = [8, 16, 32]
SHARE_SHAPE = (328, 200)  # the FMA contract's share cap is defined on frames of at least this size


def _times(nsc, m):
    return [0.5] if m == 2 else nsc.frame_times(m)


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    """(a, b): noise with alpha; read-only."""
    rng = np.random.default_rng(7001 + 31 * w + h)
    a, b = (rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(2))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _vectors(w, h, bs, seed=0):
    """int16 (blocks_y, blocks_x, 2), uniform in [-24, 24]; read-only."""
    nbx, nby = -(-w // bs), -(-h // bs)
    v = np.random.default_rng(9001 + seed + 131 * w + 17 * h + bs).integers(-24, 25, (nby, nbx, 2)).astype(np.int16)
    v.setflags(write=False)
    return v


_oracle = None


@functools.lru_cache(maxsize=None)
def _want(w, h, bs, t):
    """The oracle's frame of (_frames, _vectors) at t, computed once for every test that needs it; read-only."""
    a, b = _frames(w, h)
    out = _oracle.warp_blend(a, b, bmref.dense_flow(_vectors(w, h, bs), w, h, bs), t)
    out.setflags(write=False)
    return out


@pytest.fixture(autouse=True)
def _bind_oracle(oracle_mod):
    global _oracle
    _oracle = oracle_mod


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _warp(nsc, a, b, vec, bs, times, mode):
    """One pair, host arrays in -> (n_times, h, w, 4) from a guarded tensor."""
    import torch

    h, w = a.shape[:2]
    bm = nsc.BlockMatcher(block_size=bs, search_radius=24)
    da, db, dv = put(np.ascontiguousarray(a)), put(np.ascontiguousarray(b)), put(np.ascontiguousarray(vec))
    out = guarded.empty((len(times), h, w, 4), dtype=torch.uint8, device="cuda:0")
    fb = w * h * 4
    bm.warp_device(da.data_ptr(), fb, db.data_ptr(), fb, w, h, 1, dv.data_ptr(), out.data_ptr(), times=times, mode=mode, stream=_stream())
    return fetch(out)


def _fma_contract(got, want, share, a, b, flow, t):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print(f"fma: max |diff| {d.max()}, bytes differing {(d != 0).sum()} of {d.size} ({(d != 0).mean():.5%})")
    assert d.max() <= 1, d.max()
    if share:
        assert (d != 0).sum() < 0.001 * d.size, (d != 0).mean()
    h, w = a.shape[:2]  # the float64 contract (tests/_warp64.py); frames below 2 x 2 run EXACT arithmetic
    warp_contract(got, a, b, flow, t, 0.5 if min(w, h) >= 2 else 1.0, ("bm warp", (w, h), t))


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_exact_is_the_oracle_and_fma_holds_its_contract(nsc, w, h, bs):
    a, b = _frames(w, h)
    vec = _vectors(w, h, bs)
    for m in (2, 4, 8):
        times = _times(nsc, m)
        exact = _warp(nsc, a, b, vec, bs, times, "exact")
        fma = _warp(nsc, a, b, vec, bs, times, "fma")
        for k, t in enumerate(times):
            assert np.array_equal(exact[k], _want(w, h, bs, t)), (w, h, bs, m, k, "exact")
            _fma_contract(fma[k], _want(w, h, bs, t), (w, h) == SHARE_SHAPE, a, b, bmref.dense_flow(vec, w, h, bs), t)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_multi_time_call_equals_the_single_time_calls(nsc, w, h, bs):
    a, b = _frames(w, h)
    vec = _vectors(w, h, bs)
    for mode in ("exact", "fma"):
        for m in (4, 8):
            times = _times(nsc, m)
            multi = _warp(nsc, a, b, vec, bs, times, mode)
            for k, t in enumerate(times):
                assert np.array_equal(_warp(nsc, a, b, vec, bs, [t], mode)[0], multi[k]), (w, h, bs, mode, m, k)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_end_times_and_the_zero_field(nsc, oracle_mod, w, h, bs):
    a, b = _frames(w, h)
    vec = _vectors(w, h, bs)
    zero = np.zeros_like(vec)
    for mode in ("exact", "fma"):
        # t = 0 samples A at the pixel itself and weighs B with 0, t = 1 the other way round: the frames themselves
        ends = _warp(nsc, a, b, vec, bs, [0.0, 1.0], mode)
        assert np.array_equal(ends[0], a) and np.array_equal(ends[0], _want(w, h, bs, 0.0)), (w, h, bs, mode)
        assert np.array_equal(ends[1], b) and np.array_equal(ends[1], _want(w, h, bs, 1.0)), (w, h, bs, mode)
        assert np.array_equal(_warp(nsc, a, b, vec, bs, [0.0], mode)[0], a) and np.array_equal(_warp(nsc, a, b, vec, bs, [1.0], mode)[0], b)
        # an all-zero field is the zero-flow blend, byte for byte (integer sample positions: nothing to round in either mode)
        times = _times(nsc, 4)
        got = _warp(nsc, a, b, zero, bs, times, mode)
        for k, t in enumerate(times):
            assert np.array_equal(got[k], oracle_mod.warp_blend(a, b, None, t)), (w, h, bs, mode, k)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("v", [(6, -4), (-24, 24)])
def test_constant_even_vector_rolls_the_interior(nsc, bs, v):
    """B = A moved by v (even): at t = 0.5 both samples are A's pixel at p - v / 2, so away from the border the frame is A rolled
    by v / 2, byte for byte in both modes."""
    w, h = 200, 72
    a = _frames(w, h)[0]
    b = np.roll(a, (v[1], v[0]), (0, 1))
    vec = np.empty((-(-h // bs), -(-w // bs), 2), np.int16)
    vec[...] = v
    want = np.roll(a, (v[1] // 2, v[0] // 2), (0, 1))
    m = 24  # every sample of these pixels stays inside both frames and off the rolled-in seam
    for mode in ("exact", "fma"):
        got = _warp(nsc, a, b, vec, bs, [0.5], mode)[0]
        assert np.array_equal(got[m:h - m, m:w - m], want[m:h - m, m:w - m]), (bs, v, mode)


@pytest.mark.parametrize("w,h,bs", [(200, 72, 16), (33, 17, 8), (328, 200, 32)])
def test_batch_as_a_sliding_stream_with_poisoned_gaps(nsc, w, h, bs):
    """3 pairs over 4 frames a_stride apart (b = a + a_stride), their frames out_pair_stride apart: pair i's frames are the
    one-pair call's, in both modes, and neither the gaps between the pairs' outputs nor the guard bands are written."""
    import torch

    n, K = 3, 3
    fb, in_gap, out_gap = w * h * 4, 4 * 5, 4 * 37
    stride, out_stride = fb + in_gap, K * fb + out_gap
    rng = np.random.default_rng(77 + w)
    frames = np.full((n + 1, stride), 0xEE, np.uint8)
    frames[:, :fb] = rng.integers(0, 256, (n + 1, fb), dtype=np.uint8)
    vec = np.stack([_vectors(w, h, bs, seed=i) for i in range(n)])
    nb = vec.shape[1] * vec.shape[2]
    d_frames, d_vec = put(frames), put(vec)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=24)
    times = nsc.frame_times(K + 1)
    for mode in ("exact", "fma"):
        out = guarded.full((n, out_stride), 0x5C, dtype=torch.uint8, device="cuda:0")
        bm.warp_device(d_frames.data_ptr(), stride, d_frames.data_ptr() + stride, stride, w, h, n, d_vec.data_ptr(), out.data_ptr(),
                       times=times, mode=mode, out_pair_stride=out_stride, stream=_stream())
        got = fetch(out)
        assert (got[:, K * fb:] == 0x5C).all(), "the gap between the pairs' outputs was written"
        for i in range(n):
            one = guarded.empty((K, h, w, 4), dtype=torch.uint8, device="cuda:0")
            bm.warp_device(d_frames.data_ptr() + i * stride, stride, d_frames.data_ptr() + (i + 1) * stride, stride, w, h, 1,
                           d_vec.data_ptr() + i * nb * 4, one.data_ptr(), multiplier=K + 1, mode=mode, stream=_stream())
            assert np.array_equal(fetch(one).reshape(-1), got[i, :K * fb]), (mode, i)
        if mode == "exact":
            for i in range(n):
                a, b = frames[i, :fb].reshape(h, w, 4), frames[i + 1, :fb].reshape(h, w, 4)
                flow = bmref.dense_flow(vec[i], w, h, bs)
                for k, t in enumerate(times):
                    assert np.array_equal(got[i, k * fb:(k + 1) * fb].reshape(h, w, 4), _oracle.warp_blend(a, b, flow, t)), (i, k)
    assert np.array_equal(fetch(d_frames), frames), "the input stream was written"


@pytest.mark.parametrize("w,h", [(33, 17), (34, 18), (1, 9)])  # one pixel per lane, two pixels per lane, the _tiny pair
def test_block_vector_route_writes_the_dense_route_bytes(nsc, w, h):
    """k_bm_warp and k_warp_blend_flow are one tile body fed from two sources, so nus_bm_warp_device and
    nus_interp_interpolate_multi_device given the expanded vectors as an f32 flow write the same bytes: in EXACT and in FMA mode,
    at times with full mantissas (no product is exact), as one two-time call and as a single-time call."""
    import torch

    bs, times = 8, [float(np.float32(0.31415927)), float(np.float32(0.70710677))]
    a, b = _frames(w, h)
    vec = _vectors(w, h, bs)
    fb = w * h * 4
    da, db = put(np.ascontiguousarray(a)), put(np.ascontiguousarray(b))
    d_flow = put(np.ascontiguousarray(bmref.dense_flow(vec, w, h, bs)))
    it = nsc.WgpuFrameInterpolator()
    for mode in ("exact", "fma"):
        it.set_mode(mode)
        for ts in (times, times[:1]):
            dense = guarded.empty((len(ts), h, w, 4), dtype=torch.uint8, device="cuda:0")
            it.interpolate_multi_device(da.data_ptr(), fb, db.data_ptr(), fb, d_flow.data_ptr(), w, h, ts, dense.data_ptr(), 0, 1, _stream())
            assert np.array_equal(_warp(nsc, a, b, vec, bs, ts, mode), fetch(dense)), (w, h, mode, len(ts))
