"""The metrics entry points without a device (nus_metrics_*, nu_scaler_amd.metrics, both command-line parsers): symbols, enum
values, signatures, workspace sizes and every argument check, which runs before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "nuscaler_hip.h")
FB = 64 * 48 * 4  # one 64 x 48 frame


def test_header_declares_the_entry_points_and_the_mask():
    text = open(HEADER).read()
    assert re.search(r"^\s*NUS_METRIC_MSE = 1,$", text, re.M) and re.search(r"^\s*NUS_METRIC_SSIM = 2$", text, re.M)
    for name in ("nus_metrics_workspace_size", "nus_metrics_compare_device", "nus_metrics_compare"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "common.rs:475-543" in text


def test_bindings(nsc):
    C = nsc._capi
    assert (C.METRIC_MSE, C.METRIC_SSIM) == (1, 2)
    sig = {n: (r, a) for n, r, a in C.SIGNATURES}
    assert sig["nus_metrics_workspace_size"] == (ctypes.c_size_t, [ctypes.c_uint32] * 3 + [ctypes.c_int])
    assert len(sig["nus_metrics_compare_device"][1]) == 12 and sig["nus_metrics_compare_device"][0] is ctypes.c_int
    assert len(sig["nus_metrics_compare"][1]) == 9
    L = C.lib()
    for n in sig:
        if n.startswith("nus_metrics_"):
            assert hasattr(L, n)
    assert nsc.ErrorMetrics is nsc.metrics.ErrorMetrics and "ErrorMetrics" in nsc.__all__


def test_workspace_size(nsc):
    L = nsc._capi.lib()
    for what in (1, 2, 3):
        one = L.nus_metrics_workspace_size(1920, 1080, 1, what)
        assert one > 0
        assert L.nus_metrics_workspace_size(1920, 1080, 8, what) == 8 * one
        assert L.nus_metrics_workspace_size(3840, 2160, 1, what) > one
    assert L.nus_metrics_workspace_size(1, 1, 1, 1) > 0
    assert nsc.metrics.workspace_size(64, 48, 2) == L.nus_metrics_workspace_size(64, 48, 2, 3)
    for args in ((0, 10, 1, 1), (10, 0, 1, 1), (10, 10, 0, 1), (20, 20, 1, 0), (20, 20, 1, 4), (20, 20, 1, -1), (10, 20, 1, 2),
                 (20, 10, 1, 3)):
        assert L.nus_metrics_workspace_size(*args) == 0, args
        assert nsc._capi.last_error().startswith("nus_metrics_workspace_size:"), args
    with pytest.raises(ValueError, match="11 x 11"):
        nsc.metrics.workspace_size(10, 40, 1, mse=False, ssim=True)


def test_batches_beyond_one_launch_are_argument_errors(nsc):
    """One 1-D launch holds at most 2^32 - 1 work-items, 2^24 - 1 workgroups of 256: a batch that needs more is refused before
    any HIP call, not left to fail inside the launch."""
    L, C = nsc._capi.lib(), nsc._capi
    assert L.nus_metrics_workspace_size(1, 1, (1 << 24) - 1, 1) > 0
    for frames in (1 << 24, 20_000_000):
        assert L.nus_metrics_workspace_size(1, 1, frames, 1) == 0
        assert "too many for one launch" in C.last_error()
    big = (1 << 24) // 8 + 1  # 8 SSIM tiles (4 x 2 of 64 x 32 centres) per 266 x 74 frame
    assert L.nus_metrics_workspace_size(256 + 10, 64 + 10, big, 3) == 0 and "too many" in C.last_error()
    assert _device_call(nsc, w=1, h=1, a_stride=4, b_stride=4, frames=1 << 24, what=1, ws_bytes=1 << 40) == C.ERR_INVALID_ARGUMENT
    assert "too many for one launch" in C.last_error()


# (description, argument overrides, status, text in nus_last_error)
P = 0x10000  # a 4-byte-aligned fake device address: every case below fails before the address is used
DEVICE_CASES = [
    ("null A", dict(d_a=None), -1, "null pointer"),
    ("null B", dict(d_b=None), -1, "null pointer"),
    ("null workspace", dict(ws=None), -1, "null pointer"),
    ("null out", dict(out=None), -1, "null pointer"),
    ("misaligned A", dict(d_a=P + 2), -1, "multiples of 4"),
    ("misaligned B", dict(d_b=P + 1), -1, "multiples of 4"),
    ("misaligned A stride", dict(a_stride=FB + 2), -1, "multiples of 4"),
    ("misaligned B stride", dict(b_stride=FB + 6), -1, "multiples of 4"),
    ("misaligned out", dict(out=P + 4), -1, "8-byte aligned"),
    ("A stride below a frame", dict(a_stride=FB - 4), -1, "smaller than"),
    ("B stride below a frame", dict(b_stride=FB - 4), -1, "smaller than"),
    ("zero width", dict(w=0), -1, "non-zero"),
    ("zero height", dict(h=0), -1, "non-zero"),
    ("zero frames", dict(frames=0), -1, "non-zero"),
    ("empty mask", dict(what=0), -1, "what must be"),
    ("unknown bits", dict(what=5), -1, "what must be"),
    ("SSIM below 11 x 11", dict(w=10, h=48, a_stride=10 * 48 * 4, b_stride=10 * 48 * 4, what=3), -1, "11 x 11"),
    ("workspace too small", dict(ws_bytes=8), -1, "workspace of 8 bytes"),
]


def _device_call(nsc, **kw):
    a = dict(d_a=P, a_stride=FB, d_b=P, b_stride=FB, w=64, h=48, frames=2, what=3, ws=P, ws_bytes=None, out=P, stream=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = nsc._capi.lib().nus_metrics_workspace_size(64, 48, 2, 3)
    return nsc._capi.lib().nus_metrics_compare_device(a["d_a"], a["a_stride"], a["d_b"], a["b_stride"], a["w"], a["h"], a["frames"],
                                                      a["what"], a["ws"], a["ws_bytes"], a["out"], a["stream"])


@pytest.mark.parametrize("desc,kw,status,text", DEVICE_CASES, ids=[c[0] for c in DEVICE_CASES])
def test_device_entry_point_checks(nsc, desc, kw, status, text):
    assert _device_call(nsc, **kw) == status
    msg = nsc._capi.last_error()
    assert msg.startswith("nus_metrics_compare_device:") and text in msg, msg


def _host_call(nsc, a, b, w, h, what=3, device=0, out=True):
    res = (ctypes.c_double * 3)()
    pa = a.ctypes.data if a is not None else None
    pb = b.ctypes.data if b is not None else None
    return nsc._capi.lib().nus_metrics_compare(device, pa, a.nbytes if a is not None else 0, pb, b.nbytes if b is not None else 0,
                                               w, h, what, res if out else None)


def test_host_entry_point_checks(nsc):
    C = nsc._capi
    a = np.zeros((48, 64, 4), np.uint8)
    b = np.zeros((48, 64, 4), np.uint8)
    assert _host_call(nsc, None, b, 64, 48) == C.ERR_INVALID_ARGUMENT and "null pointer" in C.last_error()
    assert _host_call(nsc, a, None, 64, 48) == C.ERR_INVALID_ARGUMENT
    assert _host_call(nsc, a, b, 64, 48, out=False) == C.ERR_INVALID_ARGUMENT
    assert _host_call(nsc, a, b, 64, 48, what=0) == C.ERR_INVALID_ARGUMENT and "what must be" in C.last_error()
    assert _host_call(nsc, a, b, 64, 48, what=8) == C.ERR_INVALID_ARGUMENT
    assert _host_call(nsc, a, b, 0, 48) == C.ERR_INVALID_ARGUMENT and "non-zero" in C.last_error()
    small = np.zeros((10, 10, 4), np.uint8)
    assert _host_call(nsc, small, small, 10, 10, what=3) == C.ERR_INVALID_ARGUMENT and "11 x 11" in C.last_error()
    # the reference's text for different sizes (common.rs:486-488), the house wording for a size that is not w*h*4
    c = np.zeros((48, 63, 4), np.uint8)
    assert _host_call(nsc, a, c, 64, 48) == C.ERR_SIZE_MISMATCH
    assert C.last_error() == "Images must have the same dimensions"
    assert _host_call(nsc, c, c, 64, 48) == C.ERR_SIZE_MISMATCH
    assert C.last_error() == "Input data size (12096) does not match expected input buffer size (12288 for 64x48)"


def test_valid_calls_without_a_device(nsc):
    C = nsc._capi
    if C.device_count() > 0:
        pytest.skip("a device is present")
    assert _device_call(nsc) == C.ERR_NO_DEVICE and "no HIP device" in C.last_error()
    assert _device_call(nsc, what=1, frames=1) == C.ERR_NO_DEVICE
    a = np.zeros((48, 64, 4), np.uint8)
    assert _host_call(nsc, a, a, 64, 48) == C.ERR_NO_DEVICE
    with pytest.raises(RuntimeError, match="no HIP device"):
        nsc.ErrorMetrics.calculate(a, a)
    with pytest.raises(RuntimeError, match="no HIP device"):
        nsc.metrics.compare_device(P, FB, P, FB, 64, 48, 1, P, nsc.metrics.workspace_size(64, 48, 1), P)


def test_python_checks(nsc):
    a = np.zeros((48, 64, 4), np.uint8)
    with pytest.raises(ValueError, match="^Images must have the same dimensions$"):
        nsc.ErrorMetrics.calculate(a, np.zeros((48, 63, 4), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        nsc.ErrorMetrics.calculate(a.astype(np.float32), a.astype(np.float32))
    with pytest.raises(ValueError, match="8-byte aligned"):
        nsc.metrics.compare_device(P, FB, P, FB, 64, 48, 1, P, nsc.metrics.workspace_size(64, 48, 1), P + 4)
    em = nsc.ErrorMetrics(4.0, float("inf"), float("nan"))
    assert (em.mse(), em.psnr()) == (4.0, float("inf")) and em.line() == "mse=4.000000 psnr=inf ssim=nan"


def test_cli_parsers_accept_compare():
    from nu_scaler_amd import cli

    args = cli.build_parser().parse_args(["compare", "a.png", "b.png", "--device", "1"])
    assert (args.command, args.a, args.b, args.device) == ("compare", "a.png", "b.png", 1)
    src = open(os.path.join(ROOT, "nu_scaler_amd", "csrc", "cli", "nus_cli.cpp")).read()
    assert 'cmd == "compare"' in src and "nu_scaler_cli compare <a.png> <b.png> [--device N]" in src
    assert "mse=%.6f psnr=%.6f ssim=%.6f" in src


def test_native_cli_usage_lists_compare(nsc):
    import subprocess

    cli = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    if not os.path.exists(cli):
        pytest.skip("native CLI not built")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "nu_scaler_cli compare <a.png> <b.png> [--device N]" in r.stdout
