"""nus_bm_interpolate_multi_device_stream on the MI355X: block-matched frame generation over a device-resident stream.  For every
pair the vectors are the yardstick's (tests/_blockmatch.py), EXACT frames are byte for byte what nus_bm_interpolate returns for
that pair -- at every batch position and for every batch size -- and FMA frames hold the interpolation path's contract against
the oracle's warp of the yardstick flow.  Streams of 5 frames at 200 x 72 and 328 x 200: a shifting sine gradient, an unrelated
pair, the moving box, shifted noise.  Every device output lives in a conftest.guarded tensor and comes down through nus_download."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _blockmatch as bmref
from _warp64 import warp_contract
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

CASES = [(200, 72, 16, 16), (200, 72, 8, 24), (328, 200, 16, 16), (328, 200, 8, 24)]  # w, h, block size, radius
N_FRAMES = 5


def _noise(w, h, seed):
    return np.random.default_rng(seed + 31 * w + h).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _gradient(w, h, shift):
    x = np.arange(w, dtype=np.float64)[None, :] - shift
    y = np.arange(h, dtype=np.float64)[:, None]
    v = 127.5 + 45 * np.sin(x / 3.0) * np.cos(y / 4.0) + 50 * np.sin((x + 2 * y) / 23.0) + 25 * np.sin(x / 9.0 + y / 11.0)
    img = np.empty((h, w, 4), np.uint8)
    img[..., 0] = np.clip(v, 0, 255)
    img[..., 1] = np.clip(255 - v, 0, 255)
    img[..., 2] = np.clip(v * 0.5 + 40, 0, 255)
    img[..., 3] = 255
    return img


@functools.lru_cache(maxsize=None)
def _stream_frames(w, h):
    """(5, h, w, 4), read-only: gradient, gradient shifted by 6, the box on noise, the box moved by 14, that frame rolled by (3, -5).
    Pair 0 is smooth motion, pair 1 unrelated content, pair 2 motion that is not smooth, pair 3 a translation."""
    bg, box = _noise(w, h, 4), _noise(w, h, 5)
    a, b = bg.copy(), bg.copy()
    bw, bh = max(w // 4, 1), max(h // 3, 1)
    x0, y0 = w // 3, h // 3
    a[y0:y0 + bh, x0:x0 + bw] = box[:bh, :bw]
    x1 = min(x0 + 14, w - bw)
    b[y0:y0 + bh, x1:x1 + bw] = box[:bh, :bw]
    c = np.roll(b, (3, -5), (0, 1))
    c[..., 3] = 255 - b[..., 3]  # alpha is ignored by the search
    f = np.stack([_gradient(w, h, 0.0), _gradient(w, h, 6.0), a, b, c])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _yardstick(w, h, bs, R):
    """Per pair of _stream_frames: the vectors after the confidence pass.  Computed once; read-only."""
    f = _stream_frames(w, h)
    with ThreadPoolExecutor(N_FRAMES - 1) as pool:  # (the search of one 328 x 200 pair at 8 / 24 takes seconds: the pairs side by side)
        v = np.stack(list(pool.map(lambda k: bmref.refine(bmref.vectors(f[k], f[k + 1], bs, R, bmref.CENTER)[0])[0], range(N_FRAMES - 1))))
    v.setflags(write=False)
    return v


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _run(bm, frames, times, mode, *, vectors=True, frame_gap=0, mid_gap=0, n_frames=None):
    """frames: (n, h, w, 4) host -> (mid (n_pairs, n_times, h, w, 4), vectors (n_pairs, by, bx, 2) or None), from guarded tensors;
    the gaps of both strides are poisoned and checked."""
    import torch

    n, h, w = frames.shape[:3]
    n_frames = n if n_frames is None else n_frames
    n_pairs = max(n_frames - 1, 0)
    fb, K = w * h * 4, len(times)
    stride, mid_stride = fb + frame_gap, K * fb + mid_gap
    buf = np.full((n, stride), 0xEE, np.uint8)
    buf[:, :fb] = frames.reshape(n, fb)
    d_frames = put(buf)
    ws_bytes = bm.stream_workspace_size(w, h, n_frames)
    ws = guarded.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    nbx, nby = bm.block_grid(w, h)
    vec = guarded.empty((max(n_pairs, 1), nby, nbx, 2), dtype=torch.int16, device="cuda:0") if vectors else None
    mid = guarded.full((max(n_pairs, 1), mid_stride), 0x5C, dtype=torch.uint8, device="cuda:0")
    bm.interpolate_stream_device(d_frames.data_ptr(), stride, n_frames, w, h, ws.data_ptr(), ws_bytes, mid.data_ptr(), times=times, mode=mode,
                                 d_vectors=vec.data_ptr() if vectors else 0, mid_pair_stride=mid_stride if mid_gap else 0,
                                 stream=_stream())
    got = fetch(mid)
    assert (got[:, K * fb:] == 0x5C).all(), "the gap between the pairs' frames was written"
    assert np.array_equal(fetch(d_frames), buf), "the input stream was written"
    if n_pairs == 0:
        assert (got == 0x5C).all(), "nothing may be written for a stream without a pair"
        return None, None
    return got[:n_pairs, :K * fb].reshape(n_pairs, K, h, w, 4), (fetch(vec) if vectors else None)


def _host_frames(bm, a, b, w, h, times, mode, **kw):
    return np.stack([np.frombuffer(x, np.uint8).reshape(h, w, 4) for x in bm.interpolate(a, b, w, h, times=times, mode=mode, **kw)])


def _fma_contract(got, want, share, a, b, flow, t):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print(f"fma: max |diff| {d.max()}, bytes differing {(d != 0).sum()} of {d.size} ({(d != 0).mean():.5%})")
    assert d.max() <= 1, d.max()
    if share:  # the cap is defined on frames of at least 328 x 200
        assert (d != 0).sum() < 0.001 * d.size, (d != 0).mean()
    warp_contract(got, a, b, flow, t, 0.5, ("bm stream", a.shape[1::-1], t))  # the float64 contract (tests/_warp64.py)


@pytest.mark.parametrize("w,h,bs,R", CASES)
def test_vectors_and_exact_frames_equal_the_pairwise_host_entry(nsc, w, h, bs, R):
    frames = _stream_frames(w, h)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R)
    for m in (2, 4):
        times = [0.5] if m == 2 else nsc.frame_times(4)
        mid, vec = _run(bm, frames, times, "exact")
        assert np.array_equal(vec, _yardstick(w, h, bs, R)), (m, "vectors")
        for k in range(N_FRAMES - 1):
            assert np.array_equal(mid[k], _host_frames(bm, frames[k], frames[k + 1], w, h, times, "exact")), (m, k)
        without, none = _run(bm, frames, times, "exact", vectors=False)  # the vectors live in the workspace: the same frames
        assert none is None and np.array_equal(without, mid), m


@pytest.mark.parametrize("w,h,bs,R", CASES)
def test_fma_frames_hold_the_contract_against_the_oracle(nsc, oracle_mod, w, h, bs, R):
    frames = _stream_frames(w, h)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R)
    times = nsc.frame_times(4)
    mid, vec = _run(bm, frames, times, "fma")
    assert np.array_equal(vec, _yardstick(w, h, bs, R))
    exact, _ = _run(bm, frames, times, "exact")
    for k in range(N_FRAMES - 1):
        flow = bmref.dense_flow(_yardstick(w, h, bs, R)[k], w, h, bs)
        for j, t in enumerate(times):
            want = oracle_mod.warp_blend(frames[k], frames[k + 1], flow, t)
            assert np.array_equal(exact[k, j], want), (k, j)
            _fma_contract(mid[k, j], want, (w, h) == (328, 200), frames[k], frames[k + 1], flow, t)


def test_every_batch_size_and_position_gives_the_same_bytes(nsc):
    w, h, bs, R = 200, 72, 16, 16
    frames = _stream_frames(w, h)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R)
    times = nsc.frame_times(4)
    for mode in ("exact", "fma"):
        whole, vec = _run(bm, frames, times, mode)
        for first in range(N_FRAMES - 1):
            for n in range(2, N_FRAMES - first + 1):
                part, pvec = _run(bm, frames[first:first + n], times, mode)
                assert np.array_equal(part, whole[first:first + n - 1]), (mode, first, n)
                assert np.array_equal(pvec, vec[first:first + n - 1]), (mode, first, n)


def test_strides_with_poisoned_gaps(nsc):
    w, h, bs, R = 200, 72, 8, 24
    frames = _stream_frames(w, h)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R)
    times = nsc.frame_times(4)
    for mode in ("exact", "fma"):
        packed, vec = _run(bm, frames, times, mode)
        gapped, gvec = _run(bm, frames, times, mode, frame_gap=4 * 37, mid_gap=4 * 11)
        assert np.array_equal(gapped, packed) and np.array_equal(gvec, vec), mode


def test_workspace_and_short_streams(nsc):
    import torch

    w, h = 200, 72
    frames = _stream_frames(w, h)
    bm = nsc.BlockMatcher("medium")
    fb = w * h * 4
    need = bm.stream_workspace_size(w, h, N_FRAMES)
    d_frames = put(np.ascontiguousarray(frames))
    ws = guarded.empty(need, dtype=torch.uint8, device="cuda:0")
    mid = guarded.full((N_FRAMES - 1, fb), 0x5C, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="nus_bm_stream_workspace_size"):
        bm.interpolate_stream_device(d_frames.data_ptr(), fb, N_FRAMES, w, h, ws.data_ptr(), need - 1, mid.data_ptr(), multiplier=2,
                                     stream=_stream())
    assert (fetch(mid) == 0x5C).all()
    for n_frames in (0, 1):  # NUS_OK, nothing launched, d_mid untouched (_run checks it)
        _run(bm, frames, [0.5], "exact", n_frames=n_frames)


def test_scene_detection_repeats_the_nearer_frame_across_a_cut(nsc):
    import _scenecut as sc

    w, h, bs, R = 200, 72, 16, 16
    frames = np.stack([_gradient(w, h, 6.0 * k) for k in range(N_FRAMES)])
    frames[2] = 0  # one frame replaced by unrelated content: the pairs on both sides of it are cuts under the defaults
    frames[2, ..., 3] = 255
    cut = [sc.is_cut(*sc.measures(frames[k], frames[k + 1]), w, h) for k in range(N_FRAMES - 1)]
    assert cut == [False, True, True, False]
    times = nsc.frame_times(4)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R)
    for mode in ("exact", "fma"):
        off, voff = _run(bm, frames, times, mode)
        bm.set_scene_detect(True)
        try:
            on, von = _run(bm, frames, times, mode)
            again, _ = _run(bm, frames, times, mode, vectors=False, frame_gap=4 * 3, mid_gap=4 * 5)
            host = [_host_frames(bm, frames[k], frames[k + 1], w, h, times, mode) for k in range(N_FRAMES - 1)]
        finally:
            bm.set_scene_detect(False)
        assert np.array_equal(von, voff), "the detector does not touch the vectors"
        assert np.array_equal(again, on), mode
        for k in range(N_FRAMES - 1):
            if mode == "exact":
                assert np.array_equal(on[k], host[k]), (mode, k)  # interpolate(..., scene detection on), pair by pair
            if cut[k]:
                for j, t in enumerate(times):
                    assert np.array_equal(on[k, j], frames[k] if t < 0.5 else frames[k + 1]), (mode, k, j)
            else:
                assert np.array_equal(on[k], off[k]), (mode, k)
        again_off, _ = _run(bm, frames, times, mode)
        assert np.array_equal(again_off, off), "with detection off again no byte differs"
