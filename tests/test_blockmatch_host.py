"""The block-matching entry points without a GPU: every argument check of nus_bm_* returns before any HIP call (the fake device
addresses below are never touched) with a text that names the entry point, the size mismatch of the host entry points is
nus_interp_interpolate's status and text, workspace and block-grid arithmetic, the rank tables' contract as seen through the
Python mirror, PyFrameInterpolator's names, quality strings and error texts, and the usage errors of both CLIs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

DA, DB, DWS, DVEC, DSAD, DFLAGS, DFLOW = (0x7F0000000000 + k * 0x10000000 for k in range(7))  # fake, 256-byte aligned
W, H = 64, 32
FB = W * H * 4


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


@pytest.fixture
def bm(lib):
    h = lib.nus_bm_create()
    assert h
    yield h
    lib.nus_bm_destroy(h)


def _err(lib, h):
    return lib.nus_bm_last_error(h).decode()


def _dev(lib, h, d_a=DA, a_stride=FB, d_b=DB, b_stride=FB, w=W, hgt=H, n_pairs=1, d_ws=DWS, ws_bytes=1 << 20, d_vec=DVEC, d_sad=DSAD,
         d_flags=DFLAGS, d_flow=None, fmt=0):
    st = lib.nus_bm_estimate_device(h, d_a, a_stride, d_b, b_stride, w, hgt, n_pairs, d_ws, ws_bytes, d_vec, d_sad, d_flags, d_flow, fmt,
                                    None)
    return st, _err(lib, h)


def test_new_symbols_are_exported(nsc, lib):
    for name in ("nus_bm_create", "nus_bm_destroy", "nus_bm_set_device", "nus_bm_last_error", "nus_bm_set_params", "nus_bm_set_quality",
                 "nus_bm_set_tie_order", "nus_bm_set_refine", "nus_bm_workspace_size", "nus_bm_estimate_device", "nus_bm_estimate",
                 "nus_bm_interpolate"):
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in nsc._capi.SIGNATURES), name
    for name in ("BlockMatcher", "PyFrameInterpolator"):
        assert name in nsc.__all__ and hasattr(nsc, name)
    hdr = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    assert "#define NUS_BM_MAX_RADIUS 24\n" in hdr and "NUS_BM_TIES_SCAN = 0, NUS_BM_TIES_CENTER = 1" in hdr
    assert nsc._capi.BM_MAX_RADIUS == 24 and (nsc._capi.BM_TIES_SCAN, nsc._capi.BM_TIES_CENTER) == (0, 1)
    assert "#define NUS_ABI_VERSION 1\n" in hdr


def test_null_handle(nsc, lib):
    inv = nsc._capi.ERR_INVALID_ARGUMENT
    assert lib.nus_bm_set_params(None, 16, 16) == inv and nsc._capi.last_error() == "null handle"
    assert lib.nus_bm_set_quality(None, 0) == inv
    assert lib.nus_bm_set_tie_order(None, 0) == inv
    assert lib.nus_bm_set_refine(None, 0) == inv
    assert lib.nus_bm_set_device(None, 0) == inv
    assert lib.nus_bm_workspace_size(None, W, H, 1) == 0
    assert _dev(lib, None)[0] == inv
    assert lib.nus_bm_last_error(None) == b"null handle"
    lib.nus_bm_destroy(None)


@pytest.mark.parametrize("bs,R,text", [(0, 16, "block_size"), (4, 16, "block_size"), (12, 16, "block_size"), (64, 16, "block_size"),
                                       (16, 0, "search_radius"), (16, 25, "search_radius"), (8, 1 << 31, "search_radius")])
def test_set_params_rejects(nsc, lib, bm, bs, R, text):
    assert lib.nus_bm_set_params(bm, bs, R) == nsc._capi.ERR_INVALID_ARGUMENT
    msg = _err(lib, bm)
    assert msg.startswith("nus_bm_set_params:") and text in msg, msg
    assert nsc._capi.last_error() == msg


def test_setters(nsc, lib, bm):
    ok, inv = nsc._capi.OK, nsc._capi.ERR_INVALID_ARGUMENT
    for bs in (8, 16, 32):
        for R in (1, 7, 24):
            assert lib.nus_bm_set_params(bm, bs, R) == ok
    for q in (0, 1, 2):
        assert lib.nus_bm_set_quality(bm, q) == ok
    for q in (-1, 3):
        assert lib.nus_bm_set_quality(bm, q) == inv and _err(lib, bm).startswith("nus_bm_set_quality:")
    for o in (0, 1):
        assert lib.nus_bm_set_tie_order(bm, o) == ok
    for o in (-1, 2):
        assert lib.nus_bm_set_tie_order(bm, o) == inv and _err(lib, bm).startswith("nus_bm_set_tie_order:")
    for r in (0, 1):
        assert lib.nus_bm_set_refine(bm, r) == ok
    assert lib.nus_bm_set_refine(bm, 2) == inv and _err(lib, bm).startswith("nus_bm_set_refine:")
    assert lib.nus_bm_set_device(bm, -1) == inv and _err(lib, bm).startswith("nus_bm_set_device:")
    assert lib.nus_bm_set_device(bm, 3) == ok


def _workspace(w, h, bs, n):
    nb = -(-w // bs) * -(-h // bs)
    raw = (n * nb * 4 + 15) & ~15
    return raw + n * (-(-nb // 256)) * 4


def test_workspace_size_and_block_grid(nsc, lib, bm):
    for q, bs in ((0, 8), (1, 16), (2, 32)):
        assert lib.nus_bm_set_quality(bm, q) == nsc._capi.OK
        for w, h, n in ((1, 1, 1), (7, 5, 3), (1920, 1080, 1), (1920, 1080, 16), (3840, 2160, 2), (33, 17, 65535)):
            assert lib.nus_bm_workspace_size(bm, w, h, n) == _workspace(w, h, bs, n), (bs, w, h, n)
    m = nsc.BlockMatcher("medium")
    assert m.block_grid(1920, 1080) == (120, 68)  # the bottom block row is 8 pixels high
    assert nsc.BlockMatcher("high").block_grid(1920, 1080) == (240, 135)
    assert nsc.BlockMatcher("low").block_grid(1920, 1080) == (60, 34)
    assert m.block_grid(1, 1) == (1, 1) and m.block_grid(17, 16) == (2, 1)
    assert m.workspace_size(1920, 1080, 2) == _workspace(1920, 1080, 16, 2)
    assert (m.block_size, m.search_radius) == (16, 16)
    for w, h, n in ((0, 4, 1), (4, 0, 1), (1 << 16, 1 << 15, 1), (16, 16, 65536), (1, 8 * 65536, 1)):
        lib.nus_bm_set_quality(bm, 0)
        assert lib.nus_bm_workspace_size(bm, w, h, n) == 0
        assert _err(lib, bm).startswith("nus_bm_workspace_size:"), _err(lib, bm)
    with pytest.raises(ValueError, match="nus_bm_workspace_size"):
        m.workspace_size(0, 5)


@pytest.mark.parametrize("kw,text", [
    (dict(w=0), "bad dimensions"),
    (dict(hgt=0), "bad dimensions"),
    (dict(w=1 << 16, hgt=1 << 15), "bad dimensions"),
    (dict(n_pairs=65536), "too many"),
    (dict(w=1, hgt=16 * 65536, a_stride=0, b_stride=0), "too many"),
    (dict(d_a=None), "null device pointer"),
    (dict(d_b=None), "null device pointer"),
    (dict(d_ws=None), "null device pointer"),
    (dict(d_vec=None), "null device pointer"),
    (dict(fmt=2), "flow_format"),
    (dict(fmt=-1), "flow_format"),
    (dict(d_a=DA + 2), "pixel aligned"),
    (dict(d_b=DB + 1), "pixel aligned"),
    (dict(a_stride=FB + 2), "pixel aligned"),
    (dict(b_stride=FB + 1), "pixel aligned"),
    (dict(d_vec=DVEC + 2), "pixel aligned"),
    (dict(d_sad=DSAD + 2), "pixel aligned"),
    (dict(d_flow=DFLOW + 4), "pixel aligned"),  # f32 flow: 8-byte aligned
    (dict(d_flow=DFLOW + 2, fmt=1), "pixel aligned"),  # f16 flow: 4-byte aligned
    (dict(d_ws=DWS + 8), "workspace must be 16-byte aligned"),
    (dict(ws_bytes=0), "nus_bm_workspace_size"),
])
def test_device_entry_rejects(nsc, lib, bm, kw, text):
    st, msg = _dev(lib, bm, **kw)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert msg.startswith("nus_bm_estimate_device:") and text in msg, msg
    assert nsc._capi.last_error() == msg


def test_device_entry_workspace_bound_is_exact(nsc, lib, bm):
    need = lib.nus_bm_workspace_size(bm, W, H, 3)
    st, msg = _dev(lib, bm, n_pairs=3, ws_bytes=need - 1)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT and f"{need} needed" in msg
    # every check passes and there is nothing to launch: NUS_OK without a HIP call (this test runs without a GPU)
    for kw in (dict(), dict(d_sad=None, d_flags=None), dict(d_flow=DFLOW), dict(d_flow=DFLOW + 4, fmt=1), dict(d_flags=DFLAGS + 1)):
        st, msg = _dev(lib, bm, n_pairs=0, ws_bytes=need, **kw)
        assert st == nsc._capi.OK, (kw, msg)


def _host_estimate(lib, h, a_len=FB, b_len=FB, w=W, hgt=H, vec=True, null_a=False):
    a, b = np.zeros(max(a_len, 1), np.uint8), np.zeros(max(b_len, 1), np.uint8)
    out = np.zeros(4096, np.int16)
    st = lib.nus_bm_estimate(h, None if null_a else a.ctypes.data, a_len, b.ctypes.data, b_len, w, hgt, out.ctypes.data if vec else None,
                             None, None)
    return st, _err(lib, h)


def _host_interp(lib, h, times=(0.5,), n=None, a_len=FB, b_len=FB, w=W, hgt=H, mode=0, out_cap=None, null_out=False):
    a, b = np.zeros(max(a_len, 1), np.uint8), np.zeros(max(b_len, 1), np.uint8)
    n = len(times) if n is None else n
    cap = FB * max(n, 1) if out_cap is None else out_cap
    out = np.zeros(max(cap, 1), np.uint8)
    ts = None if times is None else (ctypes.c_float * max(len(times), 1))(*times)
    st = lib.nus_bm_interpolate(h, a.ctypes.data, a_len, b.ctypes.data, b_len, w, hgt, ts, n, mode, None if null_out else out.ctypes.data,
                                cap)
    return st, _err(lib, h)


def test_host_entries_size_mismatch_is_the_interpolators(nsc, lib, bm):
    it = lib.nus_interp_create(2)
    try:
        for a_len, b_len in ((FB - 4, FB), (FB, FB + 4), (0, 0)):
            a, b, out = np.zeros(max(a_len, 1), np.uint8), np.zeros(max(b_len, 1), np.uint8), np.zeros(FB, np.uint8)
            st1 = lib.nus_interp_interpolate(it, a.ctypes.data, a_len, b.ctypes.data, b_len, None, W, H, ctypes.c_float(0.5),
                                             out.ctypes.data, FB)
            msg1 = lib.nus_interp_last_error(it).decode()
            for st, msg in (_host_estimate(lib, bm, a_len=a_len, b_len=b_len), _host_interp(lib, bm, a_len=a_len, b_len=b_len)):
                assert st == st1 == nsc._capi.ERR_SIZE_MISMATCH
                assert msg == msg1 == (f"Expected {FB} bytes per frame for {W}x{H}x4 RGBA, got frame_a: {a_len} bytes, "
                                       f"frame_b: {b_len} bytes")
    finally:
        lib.nus_interp_destroy(it)


def test_host_estimate_rejects(nsc, lib, bm):
    inv = nsc._capi.ERR_INVALID_ARGUMENT
    st, msg = _host_estimate(lib, bm, w=0, a_len=0, b_len=0)
    assert st == inv and msg == "nus_bm_estimate: bad dimensions"
    st, msg = _host_estimate(lib, bm, vec=False)
    assert st == inv and msg == "nus_bm_estimate: vectors_out is null"
    st, msg = _host_estimate(lib, bm, null_a=True)
    assert st == inv and msg == "nus_bm_estimate: null frame pointer"


@pytest.mark.parametrize("times,n,text", [
    (None, 3, "times is null"),
    ((0.5,), 0, "n_times must be 1..7"),
    (tuple(k / 9 for k in range(1, 9)), 8, "n_times must be 1..7"),
    ((0.25, float("nan")), 2, "times[1]"),
    ((-0.01,), 1, "times[0]"),
    ((0.5, 1.0001), 2, "times[1]"),
])
def test_host_interpolate_rejects_bad_time_sets(nsc, lib, bm, times, n, text):
    st, msg = _host_interp(lib, bm, times=times, n=n, out_cap=FB * 8)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert msg.startswith("nus_bm_interpolate:") and text in msg, msg


def test_host_interpolate_rejects(nsc, lib, bm):
    inv = nsc._capi.ERR_INVALID_ARGUMENT
    st, msg = _host_interp(lib, bm, w=0, a_len=0, b_len=0)
    assert st == inv and msg == "nus_bm_interpolate: bad dimensions"
    st, msg = _host_interp(lib, bm, mode=2)
    assert st == inv and msg.startswith("nus_bm_interpolate: mode")
    st, msg = _host_interp(lib, bm, times=(0.25, 0.5, 0.75), out_cap=3 * FB - 1)
    assert st == inv and msg.startswith("nus_bm_interpolate:") and "capacity" in msg
    st, msg = _host_interp(lib, bm, null_out=True)
    assert st == inv and msg == "nus_bm_interpolate: null frame pointer"


# ---- Python ------------------------------------------------------------------------------

def test_block_matcher_arguments(nsc):
    with pytest.raises(ValueError, match="block_size"):
        nsc.BlockMatcher(block_size=10)
    with pytest.raises(ValueError, match="search_radius"):
        nsc.BlockMatcher(search_radius=0)
    with pytest.raises(ValueError, match="tie order"):
        nsc.BlockMatcher(tie_order="nearest")
    m = nsc.BlockMatcher("high")
    assert (m.block_size, m.search_radius, m.tie_order, m.refine) == (8, 24, "center", True)
    m.set_quality("LOW")
    assert (m.block_size, m.search_radius) == (32, 8)
    with pytest.raises(ValueError, match="Invalid quality setting"):
        m.set_quality("ultra")
    with pytest.raises(ValueError, match="flow format"):
        m.estimate_device(DA, FB, DB, FB, W, H, 0, DWS, 1 << 20, DVEC, flow_format="f64")
    with pytest.raises(ValueError, match="nus_bm_estimate_device: null device pointer"):
        m.estimate_device(0, FB, DB, FB, W, H, 1, DWS, 1 << 20, DVEC)
    a = bytes(FB)
    with pytest.raises(ValueError, match="Expected"):
        m.estimate(a[:-4], a, W, H)
    with pytest.raises(ValueError, match="exactly one"):
        m.interpolate(a, a, W, H)
    with pytest.raises(ValueError, match="multiplier"):
        m.interpolate(a, a, W, H, multiplier=9)
    with pytest.raises(ValueError, match="mode"):
        m.interpolate(a, a, W, H, times=[0.5], mode="fast")
    with pytest.raises(ValueError, match="Expected"):
        m.interpolate(a, a[:-4], W, H, multiplier=2)


def test_py_frame_interpolator_surface(nsc):
    P = nsc.PyFrameInterpolator
    assert P().name == "OpticalFlow" and P().quality == "medium"
    assert P("block_matching").name == "BlockMatching"
    assert P("Simplified", "HIGH").name == "BlockMatching" and P("simplified", "HIGH").quality == "high"
    assert P("optical_flow", "low").quality == "low"
    assert P("no such method", "no such quality").name == "OpticalFlow"  # unknown strings default silently
    assert P("block_matching", "no such quality").quality == "medium"
    assert P.create_best_interpolator("high").name == "OpticalFlow" and P.create_best_interpolator("high").quality == "high"
    assert P.create_best_interpolator("?").quality == "medium"
    for method in ("block_matching", "optical_flow"):
        p = P(method)
        with pytest.raises(RuntimeError, match="Interpolator not initialized"):
            p.interpolate(bytes(FB), bytes(FB), 0.5)
        p.initialize(W, H)
        with pytest.raises(RuntimeError, match="Frame size mismatch"):
            p.interpolate(bytes(FB - 4), bytes(FB), 0.5)
        with pytest.raises(RuntimeError, match="Frame size mismatch"):
            p.interpolate(bytes(FB), bytes(FB + 4), 0.5)
        p.quality = "High"
        assert p.quality == "high"
        with pytest.raises(ValueError, match="Invalid quality setting"):
            p.quality = "ultra"
        assert p.quality == "high"
    p = P("block_matching", "low")
    assert (p._bm.block_size, p._bm.search_radius) == (32, 8)
    p.quality = "high"
    assert (p._bm.block_size, p._bm.search_radius) == (8, 24)


# ---- CLIs ----------------------------------------------------------------------------------

EXCLUDE = "--method and --flow exclude each other"
USAGE_ERRORS = [(["--method", "block_matching", "--flow"], EXCLUDE), (["--flow", "--method", "block_matching", "--quality", "high"], EXCLUDE),
                (["--method", "optical"], "--method must be block_matching"),
                (["--method", "block_matching", "--quality", "ultra"], "--quality must be high, medium or low"),
                (["--method", "block_matching", "--multiplier", "9"], "--multiplier must be from 2 to 8"),
                (["--method", "block_matching", "--multiplier", "2", "--t", "0.5"], "--multiplier and --t exclude each other")]


@pytest.mark.parametrize("extra,text", USAGE_ERRORS)
def test_python_cli_usage_errors(tmp_path, extra, text):
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = str(tmp_path / "mid.png")
    r = subprocess.run([sys.executable, "-m", "nu_scaler_amd.cli", "interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png"), out]
                       + extra, capture_output=True, text=True, timeout=120, cwd=str(tmp_path), env=env)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert text in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra,text", USAGE_ERRORS)
def test_native_cli_usage_errors(nsc, tmp_path, extra, text):
    cli = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    assert os.path.exists(cli), "the native CLI is built with the library"
    out = str(tmp_path / "mid.png")
    r = subprocess.run([cli, "interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png"), out] + extra, capture_output=True,
                       text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert text in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []
