"""The multi-time interpolation entry points without a GPU: every argument check of nus_interp_interpolate_multi_device,
nus_interp_interpolate_multi and nus_flow_interpolate_multi_device_stream returns NUS_ERR_INVALID_ARGUMENT (the host entry's size
mismatch: nus_interp_interpolate's status and text) before any HIP call -- the fake device addresses below are never touched --,
frame_times, the Python wrapper's argument errors and the usage errors of both CLIs."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

DA, DB, DOUT, DFLOW = 0x7F0000000000, 0x7F0010000000, 0x7F0020000000, 0x7F0030000000  # fake, 256-byte aligned
W, H = 64, 32
FB = W * H * 4


def _times(*ts):
    return (ctypes.c_float * max(len(ts), 1))(*ts)


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


@pytest.fixture
def interp(lib):
    h = lib.nus_interp_create(2)
    assert h
    yield h
    lib.nus_interp_destroy(h)


@pytest.fixture
def flow(lib):
    h = lib.nus_flow_create()
    assert h
    yield h
    lib.nus_flow_destroy(h)


def _dev(lib, h, times=(0.25, 0.5, 0.75), n=None, d_a=DA, a_stride=FB, d_b=DB, b_stride=FB, d_flow=None, w=W, hgt=H, d_out=DOUT,
         stride=0, n_pairs=1):
    ts = None if times is None else _times(*times)
    n = len(times) if n is None else n
    st = lib.nus_interp_interpolate_multi_device(h, d_a, a_stride, d_b, b_stride, d_flow, w, hgt, ts, n, d_out, stride, n_pairs, None)
    return st, lib.nus_interp_last_error(h).decode()


def _host(lib, h, times=(0.5,), n=None, a_len=FB, b_len=FB, w=W, hgt=H, out_cap=None):
    a = np.zeros(max(a_len, 1), np.uint8)
    b = np.zeros(max(b_len, 1), np.uint8)
    n = len(times) if n is None else n
    cap = FB * max(n, 1) if out_cap is None else out_cap
    out = np.zeros(max(cap, 1), np.uint8)
    ts = None if times is None else _times(*times)
    st = lib.nus_interp_interpolate_multi(h, a.ctypes.data, a_len, b.ctypes.data, b_len, None, w, hgt, ts, n, out.ctypes.data, cap)
    return st, lib.nus_interp_last_error(h).decode()


def _flow(lib, h, times=(0.25, 0.5, 0.75), n=None, n_frames=3, w=W, hgt=H, fmt=0, d_flows=None, d_mid=DOUT, stride=0, frames=DA,
          levels=2):
    ts = None if times is None else _times(*times)
    n = len(times) if n is None else n
    st = lib.nus_flow_interpolate_multi_device_stream(h, frames, n_frames, w, hgt, levels, 4, 2, ctypes.c_float(0.0004), ts, n, fmt,
                                                      d_flows, d_mid, stride, None)
    return st, lib.nus_flow_last_error(h).decode()


BAD_TIME_SETS = [
    (None, 3, "times is null"),
    ((0.5,), 0, "n_times must be 1..7"),
    (tuple(k / 9 for k in range(1, 9)), 8, "n_times must be 1..7"),
    ((0.25, float("nan")), 2, "times[1]"),
    ((-0.01,), 1, "times[0]"),
    ((0.5, 1.0001), 2, "times[1]"),
    ((float("inf"),), 1, "times[0]"),
]


@pytest.mark.parametrize("times,n,text", BAD_TIME_SETS)
def test_device_entry_rejects_bad_time_sets(nsc, lib, interp, times, n, text):
    st, msg = _dev(lib, interp, times=times, n=n)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert msg.startswith("nus_interp_interpolate_multi_device:") and text in msg, msg


@pytest.mark.parametrize("times,n,text", BAD_TIME_SETS)
def test_host_entry_rejects_bad_time_sets(nsc, lib, interp, times, n, text):
    st, msg = _host(lib, interp, times=times, n=n, out_cap=FB * 8)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert msg.startswith("nus_interp_interpolate_multi:") and text in msg, msg


@pytest.mark.parametrize("times,n,text", BAD_TIME_SETS)
def test_flow_entry_rejects_bad_time_sets(nsc, lib, flow, times, n, text):
    st, msg = _flow(lib, flow, times=times, n=n)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert msg.startswith("nus_flow_interpolate_multi_device_stream:") and text in msg, msg


@pytest.mark.parametrize("kw,text", [
    (dict(d_a=DA + 2), "pixel aligned"),
    (dict(d_b=DB + 1), "pixel aligned"),
    (dict(d_out=DOUT + 2), "pixel aligned"),
    (dict(a_stride=FB + 2), "pixel aligned"),
    (dict(b_stride=FB + 1), "pixel aligned"),
    (dict(d_flow=DFLOW + 4), "pixel aligned"),  # f32 flow: 8-byte aligned
    (dict(stride=3 * FB - 4), "out_pair_stride"),
    (dict(stride=4 * FB + 2), "out_pair_stride"),
    (dict(w=0), "bad dimensions"),
    (dict(hgt=0), "bad dimensions"),
    (dict(w=1 << 16, hgt=1 << 15), "bad dimensions"),
    (dict(d_a=0), "null device pointer"),
    (dict(d_out=0), "null device pointer"),
])
def test_device_entry_rejects_bad_layouts(nsc, lib, interp, kw, text):
    st, msg = _dev(lib, interp, **kw)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert msg.startswith("nus_interp_interpolate_multi_device:") and text in msg, msg


def test_device_entry_accepts_display_order_stride_and_zero_pairs(nsc, lib, interp):
    # all checks pass, nothing to launch: NUS_OK without a HIP call (this test runs without a GPU)
    for stride in (0, 3 * FB, 4 * FB, 4 * FB + 4):
        st, msg = _dev(lib, interp, stride=stride, n_pairs=0)
        assert st == nsc._capi.OK, msg
    st, msg = _dev(lib, interp, times=(0.0, 1.0, 0.5, 0.5), n_pairs=0)
    assert st == nsc._capi.OK, msg


def test_device_entry_f16_flow_needs_4_byte_alignment_only(nsc, lib, interp):
    assert lib.nus_interp_set_flow_format(interp, 1) == nsc._capi.OK
    st, msg = _dev(lib, interp, d_flow=DFLOW + 4, n_pairs=0)
    assert st == nsc._capi.OK, msg
    st, msg = _dev(lib, interp, d_flow=DFLOW + 2)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT and "pixel aligned" in msg


def test_host_entry_size_mismatch_is_the_single_time_text(nsc, lib, interp):
    for a_len, b_len in ((FB - 4, FB), (FB, FB + 4), (0, 0)):
        st, msg = _host(lib, interp, times=(0.25, 0.75), a_len=a_len, b_len=b_len)
        a = np.zeros(max(a_len, 1), np.uint8)
        b = np.zeros(max(b_len, 1), np.uint8)
        out = np.zeros(FB, np.uint8)
        st1 = lib.nus_interp_interpolate(interp, a.ctypes.data, a_len, b.ctypes.data, b_len, None, W, H, ctypes.c_float(0.25),
                                         out.ctypes.data, FB)
        msg1 = lib.nus_interp_last_error(interp).decode()
        assert st == st1 == nsc._capi.ERR_SIZE_MISMATCH
        assert msg == msg1 == (f"Expected {FB} bytes per frame for {W}x{H}x4 RGBA, got frame_a: {a_len} bytes, "
                               f"frame_b: {b_len} bytes")


def test_host_entry_rejects_small_output_and_bad_dimensions(nsc, lib, interp):
    st, msg = _host(lib, interp, times=(0.25, 0.5, 0.75), out_cap=3 * FB - 1)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT and msg.startswith("nus_interp_interpolate_multi:") and "capacity" in msg
    st, msg = _host(lib, interp, w=0, a_len=0, b_len=0)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT and msg == "nus_interp_interpolate_multi: bad dimensions"


@pytest.mark.parametrize("kw,text", [
    (dict(d_mid=DOUT + 4), "16-byte aligned"),
    (dict(d_flows=DFLOW + 8), "16-byte aligned"),
    (dict(frames=DA + 2), "aligned"),
    (dict(stride=3 * FB - 4), "mid_pair_stride"),
    (dict(stride=4 * FB + 1), "mid_pair_stride"),
    (dict(w=0), "bad image dimensions"),
    (dict(w=1 << 15, hgt=1 << 14), "bad image dimensions"),
    (dict(n_frames=1), "at least 2 frames"),
    (dict(d_mid=None), "null device pointer"),
    (dict(frames=None), "null device pointer"),
])
def test_flow_entry_rejects_bad_arguments(nsc, lib, flow, kw, text):
    st, msg = _flow(lib, flow, **kw)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert msg.startswith("nus_flow_interpolate_multi_device_stream:") and text in msg, msg


def test_flow_entry_rejects_unknown_flow_format(nsc, lib, flow):
    st, _ = _flow(lib, flow, fmt=2)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    assert nsc._capi.last_error() == "nus_flow_interpolate_multi_device_stream: flow_format must be NUS_FLOW_F32 or NUS_FLOW_F16"


def test_header_and_binding_constants(nsc):
    h = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    assert "#define NUS_INTERP_MAX_TIMES 7\n" in h
    assert "#define NUS_ABI_VERSION 1\n" in h
    assert nsc._capi.INTERP_MAX_TIMES == 7


# ---- Python ------------------------------------------------------------------------------

def test_frame_times():
    from nu_scaler_amd.interpolator import frame_times

    assert frame_times(2) == [0.5]
    assert frame_times(4) == [0.25, 0.5, 0.75]
    for m in range(2, 9):
        ts = frame_times(m)
        assert len(ts) == m - 1
        assert ts == [float(np.float32(k / m)) for k in range(1, m)]
        assert all(isinstance(t, float) for t in ts)
    assert frame_times(3)[0] == float(np.float32(1 / 3)) != 1 / 3
    for bad in (0, 1, 9, 100, -4, 2.0, "4", None, True):
        with pytest.raises(ValueError):
            frame_times(bad)


def test_interpolate_multi_py_argument_errors(nsc):
    it = nsc.WgpuFrameInterpolator()
    a = bytes(FB)
    with pytest.raises(ValueError, match="exactly one"):
        it.interpolate_multi_py(a, a, W, H)
    with pytest.raises(ValueError, match="exactly one"):
        it.interpolate_multi_py(a, a, W, H, times=[0.5], multiplier=2)
    with pytest.raises(ValueError, match="multiplier"):
        it.interpolate_multi_py(a, a, W, H, multiplier=9)
    with pytest.raises(ValueError, match="multiplier"):
        it.interpolate_multi_py(a, a, W, H, multiplier=1)
    with pytest.raises(ValueError, match="between 1 and 7"):
        it.interpolate_multi_py(a, a, W, H, times=[])
    with pytest.raises(ValueError, match="between 1 and 7"):
        it.interpolate_multi_py(a, a, W, H, times=[0.1] * 8)
    for bad in (math.nan, -0.5, 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            it.interpolate_multi_py(a, a, W, H, times=[0.5, bad])
    with pytest.raises(ValueError, match="bytes of flow"):
        it.interpolate_multi_py(a, a, W, H, multiplier=2, flow=np.zeros((H, W, 1), np.float32))
    with pytest.raises(ValueError, match="Expected"):  # the library's size mismatch, as interpolate_py
        it.interpolate_multi_py(a[:-4], a, W, H, multiplier=3)


# ---- CLIs ----------------------------------------------------------------------------------

EXCLUDE, RANGE = "--multiplier and --t exclude each other", "--multiplier must be from 2 to 8"
USAGE_ERRORS = [(["--multiplier", "4", "--t", "0.5"], EXCLUDE), (["--t", "0.25", "--multiplier", "2"], EXCLUDE),
                (["--multiplier", "1"], RANGE), (["--multiplier", "9"], RANGE), (["--multiplier", "0"], RANGE),
                (["--multiplier", "-3", "--flow"], RANGE)]


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


def test_multi_output_paths():
    from nu_scaler_amd.imagefile import multi_output_paths

    assert multi_output_paths("/x/mid.png", 4) == ["/x/mid_1.png", "/x/mid_2.png", "/x/mid_3.png"]
    assert multi_output_paths("out", 2) == ["out_1"]
