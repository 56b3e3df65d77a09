"""nus_bm_warp_device, nus_bm_stream_workspace_size and nus_bm_interpolate_multi_device_stream without a GPU: the symbols and
their bindings are there, every argument check returns NUS_ERR_INVALID_ARGUMENT before any HIP call (the fake device addresses
below are never touched) with a text that names the entry point, and the stream workspace is the sum its header text states."""
import ctypes

import pytest

DA, DB, DVEC, DOUT, DWS, DMID = (0x7F0000000000 + k * 0x10000000 for k in range(6))  # fake, 256-byte aligned
W, H = 64, 32
FB = W * H * 4
WARP, STREAM, SIZER = "nus_bm_warp_device", "nus_bm_interpolate_multi_device_stream", "nus_bm_stream_workspace_size"


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


@pytest.fixture
def bm(lib):
    h = lib.nus_bm_create()
    assert h
    yield h
    lib.nus_bm_destroy(h)


def _times(times):
    return None if times is None else (ctypes.c_float * max(len(times), 1))(*times)


def _warp(lib, h, d_a=DA, a_stride=FB, d_b=DB, b_stride=FB, w=W, hgt=H, n_pairs=1, d_vec=DVEC, times=(0.5,), n=None, mode=0,
          d_out=DOUT, stride=0):
    n = len(times) if n is None else n
    st = lib.nus_bm_warp_device(h, d_a, a_stride, d_b, b_stride, w, hgt, n_pairs, d_vec, _times(times), n, mode, d_out, stride, None)
    return st, lib.nus_bm_last_error(h).decode() if h else ""


def _stream(lib, h, d_frames=DA, frame_stride=FB, n_frames=3, w=W, hgt=H, times=(0.5,), n=None, mode=0, d_ws=DWS, ws_bytes=1 << 24,
            d_vec=DVEC, d_mid=DMID, stride=0):
    n = len(times) if n is None else n
    st = lib.nus_bm_interpolate_multi_device_stream(h, d_frames, frame_stride, n_frames, w, hgt, _times(times), n, mode, d_ws, ws_bytes,
                                                    d_vec, d_mid, stride, None)
    return st, lib.nus_bm_last_error(h).decode() if h else ""


def test_symbols_bindings_and_declarations(nsc, lib):
    import os

    from conftest import ROOT

    hdr = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "nu_scaler_hip-sys", "src", "lib.rs")).read()
    for name in (WARP, SIZER, STREAM):
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in nsc._capi.SIGNATURES), name
        assert f" {name}(nus_blockmatch *h," in hdr, name
        assert f"pub fn {name}(h: *mut nus_blockmatch," in rs, name
    for name in ("warp_device", "stream_workspace_size", "interpolate_stream_device"):
        assert callable(getattr(nsc.BlockMatcher, name)), name
    assert "#define NUS_ABI_VERSION 1\n" in hdr  # the additions are additive


def test_null_handle(nsc, lib):
    inv = nsc._capi.ERR_INVALID_ARGUMENT
    assert _warp(lib, None)[0] == inv and nsc._capi.last_error() == "null handle"
    assert _stream(lib, None)[0] == inv
    assert lib.nus_bm_stream_workspace_size(None, W, H, 3) == 0


BAD_TIMES = [
    (dict(times=None, n=3), "times is null"),
    (dict(times=(0.5,), n=0), "n_times must be 1..7"),
    (dict(times=tuple(k / 9 for k in range(1, 9)), n=8), "n_times must be 1..7"),
    (dict(times=(0.25, float("nan"))), "times[1]"),
    (dict(times=(-0.01,)), "times[0]"),
    (dict(times=(0.5, 1.0001)), "times[1]"),
]


@pytest.mark.parametrize("kw,text", [
    (dict(w=0), "bad dimensions"),
    (dict(hgt=0), "bad dimensions"),
    (dict(w=1 << 16, hgt=1 << 15), "bad dimensions"),
    (dict(d_a=None), "null device pointer"),
    (dict(d_b=None), "null device pointer"),
    (dict(d_vec=None), "null device pointer"),
    (dict(d_out=None), "null device pointer"),
    (dict(d_a=DA + 2), "pixel aligned"),
    (dict(d_b=DB + 1), "pixel aligned"),
    (dict(a_stride=FB + 2), "pixel aligned"),
    (dict(b_stride=FB + 1), "pixel aligned"),
    (dict(d_vec=DVEC + 2), "pixel aligned"),
    (dict(d_out=DOUT + 2), "pixel aligned"),
    (dict(mode=2), "mode must be"),
    (dict(mode=-1), "mode must be"),
    (dict(times=(0.25, 0.5, 0.75), stride=3 * FB - 4), "out_pair_stride"),
    (dict(stride=FB + 2), "out_pair_stride"),
] + BAD_TIMES)
def test_warp_device_rejects(nsc, lib, bm, kw, text):
    st, msg = _warp(lib, bm, **kw)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert msg.startswith(WARP + ":") and text in msg, msg
    assert nsc._capi.last_error() == msg


def test_warp_device_with_nothing_to_launch_is_ok(nsc, lib, bm):
    # every check passes and there is nothing to launch: NUS_OK without a HIP call (this test runs without a GPU)
    for kw in (dict(), dict(times=(0.25, 0.5, 0.75), stride=3 * FB + 4), dict(mode=1, a_stride=FB + 4)):
        st, msg = _warp(lib, bm, n_pairs=0, **kw)
        assert st == nsc._capi.OK, (kw, msg)


def _bm_workspace(w, h, bs, n):
    nb = -(-w // bs) * -(-h // bs)
    return ((n * nb * 4 + 15) & ~15) + n * (-(-nb // 256)) * 4


def _up16(n):
    return (n + 15) & ~15


def test_stream_workspace_size(nsc, lib, bm):
    for q, bs in ((0, 8), (1, 16), (2, 32)):
        assert lib.nus_bm_set_quality(bm, q) == nsc._capi.OK
        for w, h, n_frames in ((1, 1, 2), (7, 5, 4), (200, 72, 5), (1920, 1080, 17), (33, 17, 65536)):
            n = n_frames - 1
            nb = -(-w // bs) * -(-h // bs)
            search = lib.nus_bm_workspace_size(bm, w, h, n)
            assert search == _bm_workspace(w, h, bs, n)
            base = _up16(search) + _up16(n * nb * 4)  # the search, then every pair's vectors
            assert lib.nus_bm_set_scene_detect(bm, 0, 20, 400) == nsc._capi.OK
            assert lib.nus_bm_stream_workspace_size(bm, w, h, n_frames) == base, (bs, w, h, n_frames)
            assert lib.nus_bm_set_scene_detect(bm, 1, 20, 400) == nsc._capi.OK
            scene = lib.nus_scene_workspace_size(w, h, n)
            assert scene > 0
            assert lib.nus_bm_stream_workspace_size(bm, w, h, n_frames) == base + _up16(scene) + _up16(n), (bs, w, h, n_frames)
            lib.nus_bm_set_scene_detect(bm, 0, 20, 400)
        # fewer than two frames: what one pair needs, never 0 (0 is the error value)
        assert lib.nus_bm_stream_workspace_size(bm, 64, 32, 0) == lib.nus_bm_stream_workspace_size(bm, 64, 32, 2) > 0
    for w, h, n_frames in ((0, 4, 2), (4, 0, 2), (1 << 16, 1 << 15, 2), (16, 16, 65537), (1, 8 * 65536, 2)):
        lib.nus_bm_set_quality(bm, 0)
        assert lib.nus_bm_stream_workspace_size(bm, w, h, n_frames) == 0
        assert lib.nus_bm_last_error(bm).decode().startswith(SIZER + ":"), lib.nus_bm_last_error(bm)
    m = nsc.BlockMatcher("medium")
    assert m.stream_workspace_size(200, 72, 5) == _up16(_bm_workspace(200, 72, 16, 4)) + _up16(4 * 13 * 5 * 4)
    with pytest.raises(ValueError, match=SIZER):
        m.stream_workspace_size(0, 5, 3)


@pytest.mark.parametrize("kw,text", [
    (dict(w=0), "bad dimensions"),
    (dict(hgt=0), "bad dimensions"),
    (dict(n_frames=65537), "too many"),
    (dict(w=1, hgt=16 * 65536), "too many"),
    (dict(d_frames=None), "null device pointer"),
    (dict(d_ws=None), "null device pointer"),
    (dict(d_mid=None), "null device pointer"),
    (dict(d_frames=DA + 2), "pixel aligned"),
    (dict(frame_stride=FB + 2), "pixel aligned"),
    (dict(d_vec=DVEC + 2), "pixel aligned"),
    (dict(d_mid=DMID + 1), "pixel aligned"),
    (dict(frame_stride=FB - 4), "frame_stride"),
    (dict(mode=2), "mode must be"),
    (dict(times=(0.25, 0.5, 0.75), stride=3 * FB - 4), "out_pair_stride"),
    (dict(d_ws=DWS + 8), "workspace must be 16-byte aligned"),
    (dict(ws_bytes=0), SIZER),
] + BAD_TIMES)
def test_stream_entry_rejects(nsc, lib, bm, kw, text):
    st, msg = _stream(lib, bm, **kw)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert msg.startswith(STREAM + ":") and text in msg, msg
    assert nsc._capi.last_error() == msg


def test_stream_entry_workspace_bound_is_exact_and_short_streams_are_ok(nsc, lib, bm):
    for scene in (0, 1):
        assert lib.nus_bm_set_scene_detect(bm, scene, 20, 400) == nsc._capi.OK
        need = lib.nus_bm_stream_workspace_size(bm, W, H, 4)
        st, msg = _stream(lib, bm, n_frames=4, ws_bytes=need - 1)
        assert st == nsc._capi.ERR_INVALID_ARGUMENT and f"{need} needed" in msg and SIZER in msg, msg
        # every check passes and there is no pair: NUS_OK without a HIP call (this test runs without a GPU)
        for n_frames in (0, 1):
            for kw in (dict(), dict(d_vec=None), dict(mode=1, times=(0.25, 0.75), stride=2 * FB + 8, frame_stride=FB + 4)):
                st, msg = _stream(lib, bm, n_frames=n_frames, ws_bytes=lib.nus_bm_stream_workspace_size(bm, W, H, n_frames), **kw)
                assert st == nsc._capi.OK, (n_frames, kw, msg)


def test_python_arguments(nsc):
    m = nsc.BlockMatcher("medium")
    with pytest.raises(ValueError, match="mode"):
        m.warp_device(DA, FB, DB, FB, W, H, 0, DVEC, DOUT, times=[0.5], mode="fast")
    with pytest.raises(ValueError, match="exactly one"):
        m.warp_device(DA, FB, DB, FB, W, H, 0, DVEC, DOUT)
    with pytest.raises(ValueError, match="multiplier"):
        m.interpolate_stream_device(DA, FB, 0, W, H, DWS, 1 << 20, DMID, multiplier=9)
    with pytest.raises(ValueError, match=WARP + ": null device pointer"):
        m.warp_device(0, FB, DB, FB, W, H, 1, DVEC, DOUT, multiplier=2)
    with pytest.raises(ValueError, match=STREAM + ": null device pointer"):
        m.interpolate_stream_device(DA, FB, 3, W, H, 0, 1 << 20, DMID, multiplier=4)
    m.warp_device(DA, FB, DB, FB, W, H, 0, DVEC, DOUT, multiplier=8, mode="fma")
    m.interpolate_stream_device(DA, FB, 1, W, H, DWS, m.stream_workspace_size(W, H, 1), DMID, multiplier=4)
