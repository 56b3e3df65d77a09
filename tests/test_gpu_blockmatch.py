"""The block-matching motion estimator on the MI355X: vectors, SADs, flags and the dense flow of nus_bm_estimate_device equal
tests/_blockmatch.py bit for bit (integer work: no tolerance anywhere), translations are recovered exactly and move the content
the right way through the warp, and nus_bm_interpolate's frames are the oracle's warp of the yardstick's flow.  Every device
output lives in a conftest.guarded tensor and comes down through nus_download."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _blockmatch as bmref
from _png import read_png
from conftest import ROOT, guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

PRESETS = [(8, 24), (16, 16), (32, 8)]  # High, Medium, Low
OFF_PRESETS = [(8, 1), (32, 24)]
ORDERS = [bmref.SCAN, bmref.CENTER]


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
def _pair(content, w, h):
    """(a, b) of one content; read-only arrays."""
    if content == "noise":
        a, b = _noise(w, h, 1), _noise(w, h, 2)
    elif content == "shifted":
        a = _noise(w, h, 3)
        b = np.roll(a, (3 % max(h, 1), -5 % max(w, 1)), (0, 1))
        b[..., 3] = 255 - a[..., 3]  # alpha is ignored
    elif content == "gradient":
        a, b = _gradient(w, h, 0.0), _gradient(w, h, 6.0)
    elif content == "flat":
        a = np.full((h, w, 4), 100, np.uint8)
        b = a.copy()
    elif content == "box":  # a textured box moving 14 pixels over a static textured background: motion that is not smooth
        bg = _noise(w, h, 4)
        box = _noise(w, h, 5)
        a, b = bg.copy(), bg.copy()
        bw, bh = max(w // 4, 1), max(h // 3, 1)
        x0, y0 = w // 3, h // 3
        a[y0:y0 + bh, x0:x0 + bw] = box[:bh, :bw]
        x1 = min(x0 + 14, w - bw)
        b[y0:y0 + bh, x1:x1 + bw] = box[:bh, :bw]
    else:
        raise ValueError(content)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _expected(content, w, h, bs, R, order):
    a, b = _pair(content, w, h)
    raw, sad = bmref.vectors(a, b, bs, R, order)
    ref, flags, smooth = bmref.refine(raw)
    return raw, sad, ref, flags, smooth


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _run(nsc, a, b, bs, R, order, refine=True, flow=None, stream=None, a_stride=None, b_stride=None, n_pairs=None):
    """a, b: device tensors of n pairs.  -> (vectors, sad, flags, flow or None) as numpy, from guarded tensors."""
    import torch

    n = a.shape[0] if n_pairs is None else n_pairs
    h, w = a.shape[1:3] if a.dim() == 4 else (None, None)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R, tie_order=order, refine=refine)
    nbx, nby = bm.block_grid(w, h)
    ws_bytes = bm.workspace_size(w, h, n)
    ws = guarded.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    vec = guarded.empty((n, nby, nbx, 2), dtype=torch.int16, device="cuda:0")
    sad = guarded.empty((n, nby, nbx), dtype=torch.int32, device="cuda:0")
    flags = guarded.empty((n, nby, nbx), dtype=torch.uint8, device="cuda:0")
    d_flow = None
    if flow is not None:
        d_flow = guarded.empty((n, h, w, 2), dtype=torch.float32 if flow == "f32" else torch.float16, device="cuda:0")
    fb = w * h * 4
    bm.estimate_device(a.data_ptr(), fb if a_stride is None else a_stride, b.data_ptr(), fb if b_stride is None else b_stride, w, h, n,
                       ws.data_ptr(), ws_bytes, vec.data_ptr(), sad.data_ptr(), flags.data_ptr(),
                       d_flow.data_ptr() if d_flow is not None else 0, flow or "f32", _stream() if stream is None else stream)
    return fetch(vec), fetch(sad).view(np.uint32), fetch(flags), (fetch(d_flow) if d_flow is not None else None)


def _check_parity(nsc, content, w, h, bs, R, order):
    a, b = _pair(content, w, h)
    raw, sad, ref, flags, smooth = _expected(content, w, h, bs, R, order)
    da, db = put(a[None].copy()), put(b[None].copy())
    for fmt, dt in (("f32", np.float32), ("f16", np.float16)):
        v, s, f, flow = _run(nsc, da, db, bs, R, order, flow=fmt)
        assert np.array_equal(v[0], ref), (content, w, h, bs, R, order, "vectors")
        assert np.array_equal(s[0], sad), (content, w, h, bs, R, order, "sad")
        assert np.array_equal(f[0], flags), (content, w, h, bs, R, order, "flags")
        want = bmref.dense_flow(ref, w, h, bs).astype(dt)
        assert flow.dtype == dt and np.array_equal(flow[0].view(np.uint8), want.view(np.uint8)), (content, w, h, bs, R, order, fmt)
    v, s, f, _ = _run(nsc, da, db, bs, R, order, refine=False)
    assert np.array_equal(v[0], raw) and np.array_equal(s[0], sad) and not f.any()
    return smooth


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("bs,R", PRESETS + OFF_PRESETS)
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (33, 17)])
def test_parity_small_shapes(nsc, w, h, bs, R, order):
    for content in ("noise", "shifted", "flat"):
        _check_parity(nsc, content, w, h, bs, R, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("bs,R", PRESETS + OFF_PRESETS)
@pytest.mark.parametrize("w,h", [(320, 240), (328, 200)])
def test_parity_shapes_and_settings(nsc, w, h, bs, R, order):
    _check_parity(nsc, "shifted", w, h, bs, R, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("content", ["noise", "gradient", "flat", "box"])
def test_parity_contents(nsc, content, order):
    smooth = _check_parity(nsc, content, 328, 200, 16, 16, order)
    if content == "box":
        raw, sad, ref, flags, _ = _expected(content, 328, 200, 16, 16, order)
        assert not smooth and (flags & 2).all() and (flags & 1).any(), "the moving box must make the confidence pass act"
    if content == "flat":
        raw = _expected(content, 328, 200, 16, 16, order)[0]
        if order == bmref.CENTER:
            assert not raw[:200 // 16, :328 // 16].any()  # (the partial blocks at the right / bottom edge must move back inside)
        else:
            assert tuple(raw[2, 2]) == (-16, -16)


def test_parity_box_high_and_low(nsc):
    for bs, R in ((8, 24), (32, 8)):
        _check_parity(nsc, "box", 328, 200, bs, R, bmref.CENTER)


def test_parity_1080p_medium(nsc):
    _check_parity(nsc, "shifted", 1920, 1080, 16, 16, bmref.CENTER)


def test_strides_with_poisoned_gaps(nsc):
    import torch

    w, h, n = 90, 50, 3
    fb, gap = w * h * 4, 4 * 37
    pairs = [(_noise(w, h, 10 + i), np.roll(_noise(w, h, 10 + i), (2, i - 1), (0, 1))) for i in range(n)]
    buf_a = np.full((n, fb + gap), 0xEE, np.uint8)
    buf_b = np.full((n, fb + 2 * gap), 0x11, np.uint8)
    for i, (a, b) in enumerate(pairs):
        buf_a[i, :fb] = a.reshape(-1)
        buf_b[i, :fb] = b.reshape(-1)
    da, db = put(buf_a), put(buf_b)
    bm = nsc.BlockMatcher("medium")
    nbx, nby = bm.block_grid(w, h)
    ws_bytes = bm.workspace_size(w, h, n)
    ws = guarded.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    vec = guarded.empty((n, nby, nbx, 2), dtype=torch.int16, device="cuda:0")
    sad = guarded.empty((n, nby, nbx), dtype=torch.int32, device="cuda:0")
    bm.estimate_device(da.data_ptr(), fb + gap, db.data_ptr(), fb + 2 * gap, w, h, n, ws.data_ptr(), ws_bytes, vec.data_ptr(),
                       sad.data_ptr(), 0, 0, "f32", _stream())
    v, s = fetch(vec), fetch(sad).view(np.uint32)
    for i, (a, b) in enumerate(pairs):
        raw, esad = bmref.vectors(a, b, 16, 16, bmref.CENTER)
        assert np.array_equal(v[i], bmref.refine(raw)[0]) and np.array_equal(s[i], esad), i
    assert (fetch(da)[:, fb:] == 0xEE).all() and (fetch(db)[:, fb:] == 0x11).all()


def test_batch_equals_pairs_one_by_one_and_repeats(nsc):
    w, h, n = 200, 120, 4
    a = np.stack([_noise(w, h, 20 + i) for i in range(n)])
    b = np.stack([np.roll(a[i], (i - 2, 3 * i - 4), (0, 1)) for i in range(n)])
    b[2] = _pair("box", w, h)[1]
    a[2] = _pair("box", w, h)[0]
    da, db = put(a), put(b)
    batch = _run(nsc, da, db, 8, 24, bmref.CENTER, flow="f16")
    again = _run(nsc, da, db, 8, 24, bmref.CENTER, flow="f16")
    for x, y in zip(batch, again):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "the same call twice must give the same bytes"
    for i in range(n):
        one = _run(nsc, da[i:i + 1], db[i:i + 1], 8, 24, bmref.CENTER, flow="f16")
        for x, y in zip(batch, one):
            assert np.array_equal(x[i].view(np.uint8), y[0].view(np.uint8)), i


def test_non_default_stream_is_ordered_with_a_following_warp(nsc, oracle_mod):
    import torch

    w, h = 320, 240
    a = _noise(w, h, 30)
    b = np.roll(a, (4, -6), (0, 1))
    da, db = put(a[None].copy()), put(b[None].copy())
    torch.cuda.synchronize()
    bm = nsc.BlockMatcher("medium")
    nbx, nby = bm.block_grid(w, h)
    ws_bytes = bm.workspace_size(w, h, 1)
    ws = guarded.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    vec = guarded.empty((1, nby, nbx, 2), dtype=torch.int16, device="cuda:0")
    flow = guarded.zeros((1, h, w, 2), dtype=torch.float16, device="cuda:0")
    out = guarded.empty((1, h, w, 4), dtype=torch.uint8, device="cuda:0")
    it = nsc.WgpuFrameInterpolator()
    it.set_flow_format("f16")
    s = torch.cuda.Stream()
    fb = w * h * 4
    with torch.cuda.stream(s):
        bm.estimate_device(da.data_ptr(), fb, db.data_ptr(), fb, w, h, 1, ws.data_ptr(), ws_bytes, vec.data_ptr(), 0, 0,
                           flow.data_ptr(), "f16", s.cuda_stream)
        it.interpolate_device(da.data_ptr(), fb, db.data_ptr(), fb, flow.data_ptr(), w, h, 0.5, out.data_ptr(), 1, s.cuda_stream)
        got = fetch(out)  # nus_download on the current stream: s
    raw, _ = bmref.vectors(a, b, 16, 16, bmref.CENTER)
    want = oracle_mod.warp_blend(a, b, bmref.dense_flow(bmref.refine(raw)[0], w, h, 16), 0.5)
    assert np.array_equal(got[0], want)


# ---- translation ---------------------------------------------------------------------------

TRANSLATIONS = [((12, -6), 16, 16), ((20, 10), 8, 24), ((-8, 4), 32, 8)]


def _inner_blocks(w, h, bs, R):
    """Mask of the blocks at least R + bs from every border."""
    nbx, nby = -(-w // bs), -(-h // bs)
    x0, y0 = np.arange(nbx) * bs, np.arange(nby) * bs
    okx = (x0 >= R + bs) & (x0 + bs <= w - R - bs)
    oky = (y0 >= R + bs) & (y0 + bs <= h - R - bs)
    return oky[:, None] & okx[None, :]


@pytest.mark.parametrize("s,bs,R", TRANSLATIONS)
def test_translation_is_recovered_and_moves_content_the_right_way(nsc, s, bs, R):
    w, h = 328, 248
    a = _noise(w, h, 40)
    b = np.roll(a, (s[1], s[0]), (0, 1))
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R)
    vec, sad, flags = bm.estimate(a, b, w, h)
    inner = _inner_blocks(w, h, bs, R)
    assert inner.sum() >= 4
    assert (vec[inner] == np.array(s, np.int16)).all(), "every inner block's vector is the shift, exactly"
    assert not sad[inner].any() and not (flags[inner] & 1).any()  # (bit 1 may be set: the border blocks cannot follow the shift)
    # s is even: the t = 0.5 frame is A rolled by s / 2, byte for byte, on those blocks (integer sample positions make the
    # bilinear sample and the blend exact), in both arithmetic modes
    want = np.roll(a, (s[1] // 2, s[0] // 2), (0, 1))
    px = np.repeat(np.repeat(inner, bs, 0), bs, 1)[:h, :w]
    for mode in ("exact", "fma"):
        mid = np.frombuffer(bm.interpolate(a, b, w, h, times=[0.5], mode=mode)[0], np.uint8).reshape(h, w, 4)
        assert np.array_equal(mid[px], want[px]), mode


# ---- end to end ----------------------------------------------------------------------------

def _fma_contract(got, want):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1, d.max()
    assert (d != 0).sum() < 0.001 * d.size, (d != 0).mean()


@pytest.mark.parametrize("content,bs,R", [("box", 16, 16), ("shifted", 8, 24), ("gradient", 32, 8)])
def test_interpolate_equals_the_oracle_warp_of_the_yardstick_flow(nsc, oracle_mod, content, bs, R):
    w, h = 328, 200
    a, b = _pair(content, w, h)
    flow = bmref.dense_flow(_expected(content, w, h, bs, R, bmref.CENTER)[2], w, h, bs)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R)
    times = nsc.frame_times(4)
    exact = bm.interpolate(a, b, w, h, multiplier=4, mode="exact")
    fma = bm.interpolate(a, b, w, h, multiplier=4, mode="fma")
    assert len(exact) == len(fma) == 3
    for k, t in enumerate(times):
        want = oracle_mod.warp_blend(a, b, flow, t)
        assert np.array_equal(np.frombuffer(exact[k], np.uint8).reshape(h, w, 4), want), (k, t)
        _fma_contract(np.frombuffer(fma[k], np.uint8).reshape(h, w, 4), want)
        for mode, frames in (("exact", exact), ("fma", fma)):  # multiplier 4 = three single-time calls
            assert bm.interpolate(a, b, w, h, times=[t], mode=mode)[0] == frames[k], (mode, k)


REUSE = [("shifted", 16, 12), ("noise", 48, 32), ("shifted", 16, 12)]  # the handle's device arena: small, grown, reused


def test_estimate_reuses_its_grown_arena(nsc):
    """nus_bm_estimate on one handle with a 16x12 pair (2 x 2 blocks of 8), a 48x32 pair and the 16x12 pair again: each result
    equals the yardstick bit for bit, the third the first."""
    bm = nsc.BlockMatcher(block_size=8, search_radius=24)
    got = []
    for content, w, h in REUSE:
        a, b = _pair(content, w, h)
        _, sad, ref, flags, _ = _expected(content, w, h, 8, 24, bmref.CENTER)
        v, s, f = (np.asarray(x) for x in bm.estimate(a, b, w, h))
        assert np.array_equal(v.reshape(ref.shape), ref) and np.array_equal(s.reshape(sad.shape), sad), (content, w, h)
        assert np.array_equal(f.reshape(flags.shape), flags), (content, w, h)
        got.append(v.tobytes() + s.tobytes() + f.tobytes())
    assert got[2] == got[0]


def test_interpolate_with_scene_detection_reuses_its_grown_arena(nsc, oracle_mod):
    """nus_bm_interpolate with scene detection on, same handle, same three pairs: a pair the yardstick detector flags gives
    repeats of the nearer frame, any other the oracle's warp of the yardstick flow (EXACT mode: bit for bit)."""
    import _scenecut as sc

    bm = nsc.BlockMatcher(block_size=8, search_radius=24)
    bm.set_scene_detect(True)
    times = [0.25, 0.75]
    got = []
    for content, w, h in REUSE:
        a, b = _pair(content, w, h)
        if content == "noise":  # the larger pair is a cut: noise against white
            b = np.full_like(a, 255)
            assert sc.is_cut(*sc.measures(a, b), w, h)
        if sc.is_cut(*sc.measures(a, b), w, h):
            want = [a.tobytes(), b.tobytes()]
        else:
            flow = bmref.dense_flow(_expected(content, w, h, 8, 24, bmref.CENTER)[2], w, h, 8)
            want = [oracle_mod.warp_blend(a, b, flow, t).tobytes() for t in times]
        got.append(bm.interpolate(a, b, w, h, times=times, mode="exact"))
        assert got[-1] == want, (content, w, h)
    assert got[2] == got[0]


def _write_png(path, img):
    from nu_scaler_amd.imagefile import write_png

    write_png(str(path), img.shape[1], img.shape[0], img.tobytes())


def test_pyclass_and_both_clis_give_the_library_bytes(nsc, tmp_path):
    w, h = 160, 96
    a, b = _pair("box", w, h)
    a, b = a.copy(), b.copy()
    _write_png(tmp_path / "a.png", a)
    _write_png(tmp_path / "b.png", b)
    bm = nsc.BlockMatcher("high")
    mid = bm.interpolate(a, b, w, h, times=[0.5])[0]
    three = bm.interpolate(a, b, w, h, multiplier=4)
    p = nsc.PyFrameInterpolator("block_matching", "high")
    p.initialize(w, h)
    assert p.interpolate(a.tobytes(), b.tobytes(), 0.5) == mid
    native = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    env = dict(os.environ, PYTHONPATH=ROOT)
    for tag, cmd in (("py", [sys.executable, "-m", "nu_scaler_amd.cli"]), ("native", [native])):
        one = tmp_path / f"{tag}_mid.png"
        args = ["interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png")]
        r = subprocess.run(cmd + args + [str(one), "--method", "block_matching", "--quality", "high"], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, (tag, r.stdout, r.stderr)
        assert read_png(str(one)).tobytes() == mid, tag
        r = subprocess.run(cmd + args + [str(tmp_path / f"{tag}_m.png"), "--method", "block_matching", "--quality", "high",
                                         "--multiplier", "4"], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (tag, r.stdout, r.stderr)
        for k in range(3):
            assert read_png(str(tmp_path / f"{tag}_m_{k + 1}.png")).tobytes() == three[k], (tag, k)


def test_optical_flow_pyclass_is_the_flow_estimator_and_the_warp(nsc):
    w, h = 96, 64
    a, b = _gradient(w, h, 0.0), _gradient(w, h, 1.0)
    p = nsc.PyFrameInterpolator()
    assert p.name == "OpticalFlow"
    p.initialize(w, h)
    flow = nsc.FlowEstimator().estimate(a, b, w, h)
    want = nsc.WgpuFrameInterpolator().interpolate_py(a.tobytes(), b.tobytes(), w, h, time_t=0.25, flow=flow)
    assert p.interpolate(a.tobytes(), b.tobytes(), 0.25) == want
