"""nus_flow_set_median without a GPU: the exports, the header's prototypes and bound, the ABI version, the argument check (before
any HIP call, the text begins with the entry point's name, the setting stays), the default, the primitive's argument checks, the
Python wrappers' arguments and the flag of both CLIs."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("nus_flow_set_median", "nus_flow_median_size", "nus_flow_median", "nus_flow_workspace_bytes")


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


@pytest.fixture
def flow(lib):
    h = lib.nus_flow_create()
    assert h
    yield h
    lib.nus_flow_destroy(h)


def test_exports_header_and_abi(nsc, lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in nsc._capi.SIGNATURES), name
    hdr = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    assert "#define NUS_FLOW_MEDIAN_MAX 5\n" in hdr
    assert "int nus_flow_set_median(nus_flow *h, uint32_t size);" in hdr
    assert "int nus_flow_median_size(const nus_flow *h);" in hdr
    assert "size_t nus_flow_workspace_bytes(nus_flow *h);" in hdr
    assert "int nus_flow_median(nus_flow *h, const float *flow_in, uint32_t w, uint32_t hgt, uint32_t size, float *flow_out);" in hdr
    assert "#define NUS_ABI_VERSION 1\n" in hdr
    assert lib.nus_abi_version() == 1
    assert nsc._capi.FLOW_MEDIAN_MAX == 5
    sys_rs = open(os.path.join(ROOT, "rust", "nu_scaler_hip-sys", "src", "lib.rs")).read()
    assert "pub const NUS_FLOW_MEDIAN_MAX: c_int = 5;" in sys_rs
    assert "pub fn nus_flow_set_median(h: *mut nus_flow, size: u32) -> c_int;" in sys_rs
    assert "pub fn nus_flow_median_size(h: *const nus_flow) -> c_int;" in sys_rs
    assert "pub fn nus_flow_median(h: *mut nus_flow, flow_in: *const f32, w: u32, hgt: u32, size: u32, flow_out: *mut f32) -> c_int;" in sys_rs
    assert "pub fn nus_flow_workspace_bytes(h: *mut nus_flow) -> usize;" in sys_rs
    assert "nus_k_flow_median.hip" in open(os.path.join(ROOT, "nu_scaler_amd", "csrc", "Makefile")).read()


def test_default_and_argument_check(nsc, lib, flow):
    ok, inv = nsc._capi.OK, nsc._capi.ERR_INVALID_ARGUMENT
    assert lib.nus_flow_median_size(flow) == 0
    assert lib.nus_flow_set_median(None, 3) == inv and nsc._capi.last_error() == "null handle"
    assert lib.nus_flow_median_size(None) == inv
    assert lib.nus_flow_workspace_bytes(flow) == 0 and lib.nus_flow_workspace_bytes(None) == 0  # nothing reserved yet
    for size in (0, 3, 5, 0, 5, 3):
        assert lib.nus_flow_set_median(flow, size) == ok
        assert lib.nus_flow_median_size(flow) == size
    for bad in (1, 2, 4, 6, 7, (1 << 32) - 1):
        assert lib.nus_flow_set_median(flow, bad) == inv
        msg = lib.nus_flow_last_error(flow).decode()
        assert msg.startswith("nus_flow_set_median:"), msg
        assert nsc._capi.last_error() == msg
        assert lib.nus_flow_median_size(flow) == 3  # left as it was
    assert lib.nus_flow_mode(flow) == 0 and lib.nus_flow_warps(flow) == 0  # and nothing else moved
    assert lib.nus_flow_set_warps(flow, 2) == ok and lib.nus_flow_median_size(flow) == 3  # the two settings are independent
    assert lib.nus_flow_set_median(flow, 0) == ok and lib.nus_flow_warps(flow) == 2


def test_primitive_checks_its_arguments_before_any_hip_call(nsc, lib, flow):
    inv = nsc._capi.ERR_INVALID_ARGUMENT
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    for bad in (0, 1, 2, 4, 6, 7, (1 << 32) - 1):
        assert lib.nus_flow_median(flow, p, 2, 2, bad, p) == inv
        assert lib.nus_flow_last_error(flow).decode().startswith("nus_flow_median:")
    assert lib.nus_flow_median(flow, None, 2, 2, 3, p) == inv
    assert lib.nus_flow_median(flow, p, 2, 2, 5, None) == inv
    assert lib.nus_flow_median(flow, p, 0, 2, 3, p) == inv
    assert lib.nus_flow_median(flow, p, 2, 0, 5, p) == inv
    assert lib.nus_flow_median(None, p, 2, 2, 3, p) == inv


def test_python_wrappers(nsc):
    from nu_scaler_amd.flow import FlowEstimator

    f = FlowEstimator()
    assert f.median_size == 0
    f.set_median(5)
    assert f.median_size == 5
    for bad in (-1, 1, 2, 4, 6, 7, 3.0, 2.5, True, "3"):
        with pytest.raises(ValueError, match="median"):
            f.set_median(bad)
        assert f.median_size == 5  # a rejected call changes nothing
    f.set_median(0)
    assert f.median_size == 0
    assert FlowEstimator(median=3).median_size == 3
    both = FlowEstimator(warps=2, median=5)
    assert (both.warps, both.median_size) == (2, 5)
    with pytest.raises(ValueError, match="median"):
        FlowEstimator(median=4)
    flow = np.zeros((4, 4, 2), np.float32)
    for bad in (0, 1, 4, 7, True):
        with pytest.raises(ValueError, match="median size"):
            f.median(flow, bad)
    with pytest.raises(ValueError, match="flow"):
        f.median(np.zeros((4, 4, 3), np.float32), 3)
    it = nsc.PyFrameInterpolator("optical_flow", flow_warps=1, flow_median=5)
    assert it.name == "OpticalFlow" and it._flow.median_size == 5 and it._flow.warps == 1
    assert nsc.PyFrameInterpolator("optical_flow")._flow.median_size == 0
    for method in ("block_matching", "simplified"):
        with pytest.raises(ValueError, match="flow_median"):
            nsc.PyFrameInterpolator(method, flow_median=3)
        assert nsc.PyFrameInterpolator(method, flow_median=0).name == "BlockMatching"
    for bad in (-1, 1, 4, 7):
        with pytest.raises(ValueError, match="median"):
            nsc.PyFrameInterpolator("optical_flow", flow_median=bad)


def test_imagefile_and_step_motion_arguments(nsc, tmp_path):
    import inspect

    from nu_scaler_amd import imagefile
    from nu_scaler_amd.stream import FramePipeline

    assert inspect.signature(FramePipeline.step_motion).parameters["flow_median"].default == 0
    for fn in (imagefile.interpolate_image_files, imagefile.interpolate_image_files_multi):
        assert inspect.signature(fn).parameters["flow_median"].default == 0
    missing = str(tmp_path / "a.png")  # (the checks come before anything is read)
    with pytest.raises(ValueError, match="flow_median needs estimate_flow"):
        imagefile.interpolate_image_files(missing, missing, str(tmp_path / "o.png"), 0.5, False, flow_median=3)
    with pytest.raises(ValueError, match="median"):
        imagefile.interpolate_image_files(missing, missing, str(tmp_path / "o.png"), 0.5, True, flow_median=4)
    with pytest.raises(ValueError, match="flow_median needs estimate_flow"):
        imagefile.interpolate_image_files_multi(missing, missing, str(tmp_path / "o.png"), 2, False, flow_median=5)
    with pytest.raises(ValueError, match="median"):
        imagefile.interpolate_image_files_multi(missing, missing, str(tmp_path / "o.png"), 2, True, flow_median=7)


def test_python_cli_flag(nsc, capsys):
    from nu_scaler_amd import cli

    p = cli.build_parser()
    base = ["interpolate", "a.png", "b.png", "out.png"]
    assert p.parse_args(base + ["--flow"]).flow_median is None
    assert p.parse_args(base + ["--flow", "--flow-median", "5"]).flow_median == 5
    assert p.parse_args(base + ["--flow", "--flow-warps", "1", "--flow-median", "3"]).flow_median == 3
    for argv, text in ((base + ["--flow-median", "3"], "--flow-median needs --flow"),
                       (base + ["--method", "block_matching", "--flow-median", "3"], "--flow-median needs --flow"),
                       (base + ["--flow", "--flow-median", "4"], "--flow-median must be 0, 3 or 5"),
                       (base + ["--flow", "--flow-median", "7"], "--flow-median must be 0, 3 or 5"),
                       (base + ["--flow", "--flow-median", "-1"], "--flow-median must be 0, 3 or 5")):
        with pytest.raises(SystemExit) as e:  # usage errors: status 2 before anything is read
            cli.main(argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err


@pytest.mark.parametrize("extra,text", [
    (["--flow-median", "3"], "--flow-median needs --flow"),
    (["--method", "block_matching", "--flow-median", "5"], "--flow-median needs --flow"),
    (["--flow", "--flow-median", "4"], "--flow-median must be 0, 3 or 5"),
    (["--flow", "--flow-median", "7"], "--flow-median must be 0, 3 or 5"),
    (["--flow", "--flow-median", "x"], "--flow-median must be 0, 3 or 5"),
])
def test_native_cli_usage_errors(nsc, tmp_path, extra, text):
    cli = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    assert os.path.exists(cli), "the native CLI is built with the library"
    out = str(tmp_path / "mid.png")
    r = subprocess.run([cli, "interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png"), out] + extra, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and text in r.stderr, (r.returncode, r.stderr)  # before anything is read: the frames do not exist
    assert not os.path.exists(out)
    assert "--flow-median" in r.stderr  # the usage text names the flag
