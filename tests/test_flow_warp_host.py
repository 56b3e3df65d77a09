"""nus_flow_set_warps without a GPU: the exports, the header's prototypes and bound, the ABI version, the argument check (before
any HIP call, the text begins with the entry point's name, the setting stays), the default, the Python wrappers' arguments and the
flags of both CLIs."""
import os
import subprocess

import pytest

from conftest import ROOT

NEW = ("nus_flow_set_warps", "nus_flow_warps", "nus_flow_warp_coefficients", "nus_flow_horn_schunck_coef")


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
    assert "#define NUS_FLOW_MAX_WARPS 4\n" in hdr
    assert "int nus_flow_set_warps(nus_flow *h, uint32_t warps);" in hdr
    assert "int nus_flow_warps(const nus_flow *h);" in hdr
    assert "int nus_flow_warp_coefficients(nus_flow *h, const float *i1, const float *i2, const float *flow, uint32_t w, uint32_t hgt,\n" in hdr
    assert "int nus_flow_horn_schunck_coef(nus_flow *h, const float *coef, const float *flow_in, uint32_t w, uint32_t hgt, float lambda,\n" in hdr
    assert "#define NUS_ABI_VERSION 1\n" in hdr
    assert lib.nus_abi_version() == 1
    assert nsc._capi.FLOW_MAX_WARPS == 4
    sys_rs = open(os.path.join(ROOT, "rust", "nu_scaler_hip-sys", "src", "lib.rs")).read()
    assert "pub fn nus_flow_set_warps(h: *mut nus_flow, warps: u32) -> c_int;" in sys_rs
    assert "pub fn nus_flow_warps(h: *const nus_flow) -> c_int;" in sys_rs
    assert "pub fn nus_flow_warp_coefficients(" in sys_rs and "pub fn nus_flow_horn_schunck_coef(" in sys_rs


def test_default_and_argument_check(nsc, lib, flow):
    ok, inv = nsc._capi.OK, nsc._capi.ERR_INVALID_ARGUMENT
    assert lib.nus_flow_warps(flow) == 0
    assert lib.nus_flow_set_warps(None, 1) == inv and nsc._capi.last_error() == "null handle"
    assert lib.nus_flow_warps(None) == inv
    for w in (0, 1, 2, 3, 4, 0, 3):
        assert lib.nus_flow_set_warps(flow, w) == ok
        assert lib.nus_flow_warps(flow) == w
    for bad in (5, 6, 1 << 31, (1 << 32) - 1):
        assert lib.nus_flow_set_warps(flow, bad) == inv
        msg = lib.nus_flow_last_error(flow).decode()
        assert msg.startswith("nus_flow_set_warps:"), msg
        assert nsc._capi.last_error() == msg
        assert lib.nus_flow_warps(flow) == 3  # left as it was
    assert lib.nus_flow_mode(flow) == 0  # and nothing else moved


def test_primitives_check_their_arguments_before_any_hip_call(nsc, lib, flow):
    import numpy as np

    inv = nsc._capi.ERR_INVALID_ARGUMENT
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert lib.nus_flow_warp_coefficients(flow, None, p, None, 2, 2, p) == inv
    assert lib.nus_flow_warp_coefficients(flow, p, p, None, 2, 2, None) == inv
    assert lib.nus_flow_warp_coefficients(flow, p, p, None, 0, 2, p) == inv
    assert lib.nus_flow_horn_schunck_coef(flow, None, None, 2, 2, 4e-4, 1, p) == inv
    assert lib.nus_flow_horn_schunck_coef(flow, p, None, 2, 0, 4e-4, 1, p) == inv
    assert lib.nus_flow_warp_coefficients(None, p, p, None, 2, 2, p) == inv


def test_python_wrappers(nsc):
    from nu_scaler_amd.flow import FlowEstimator

    f = FlowEstimator()
    assert f.warps == 0
    f.set_warps(2)
    assert f.warps == 2
    for bad in (-1, 5, 1.5, True):
        with pytest.raises(ValueError, match="warps"):
            f.set_warps(bad)
        assert f.warps == 2  # a rejected call changes nothing
    assert FlowEstimator(warps=3).warps == 3
    with pytest.raises(ValueError, match="warps"):
        FlowEstimator(warps=5)
    it = nsc.PyFrameInterpolator("optical_flow", flow_warps=1)
    assert it.name == "OpticalFlow" and it._flow.warps == 1
    assert nsc.PyFrameInterpolator("optical_flow")._flow.warps == 0
    for method in ("block_matching", "simplified"):
        with pytest.raises(ValueError, match="flow_warps"):
            nsc.PyFrameInterpolator(method, flow_warps=1)
        assert nsc.PyFrameInterpolator(method, flow_warps=0).name == "BlockMatching"
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="warps"):
            nsc.PyFrameInterpolator("optical_flow", flow_warps=bad)


def test_imagefile_and_step_motion_arguments(nsc, tmp_path):
    import inspect

    from nu_scaler_amd import imagefile
    from nu_scaler_amd.stream import FramePipeline

    assert inspect.signature(FramePipeline.step_motion).parameters["flow_warps"].default == 0
    for fn in (imagefile.interpolate_image_files, imagefile.interpolate_image_files_multi):
        assert inspect.signature(fn).parameters["flow_warps"].default == 0
    missing = str(tmp_path / "a.png")  # (the checks come before anything is read)
    with pytest.raises(ValueError, match="flow_warps needs estimate_flow"):
        imagefile.interpolate_image_files(missing, missing, str(tmp_path / "o.png"), 0.5, False, flow_warps=1)
    with pytest.raises(ValueError, match="warps"):
        imagefile.interpolate_image_files(missing, missing, str(tmp_path / "o.png"), 0.5, True, flow_warps=5)
    with pytest.raises(ValueError, match="flow_warps needs estimate_flow"):
        imagefile.interpolate_image_files_multi(missing, missing, str(tmp_path / "o.png"), 2, False, flow_warps=2)


def test_python_cli_flag(nsc, capsys):
    from nu_scaler_amd import cli

    p = cli.build_parser()
    base = ["interpolate", "a.png", "b.png", "out.png"]
    assert p.parse_args(base + ["--flow"]).flow_warps is None
    assert p.parse_args(base + ["--flow", "--flow-warps", "2"]).flow_warps == 2
    for argv, text in ((base + ["--flow-warps", "1"], "--flow-warps needs --flow"),
                       (base + ["--method", "block_matching", "--flow-warps", "1"], "--flow-warps needs --flow"),
                       (base + ["--flow", "--flow-warps", "5"], "--flow-warps must be from 0 to 4"),
                       (base + ["--flow", "--flow-warps", "-1"], "--flow-warps must be from 0 to 4")):
        with pytest.raises(SystemExit) as e:  # usage errors: status 2 before anything is read
            cli.main(argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err


@pytest.mark.parametrize("extra,text", [
    (["--flow-warps", "1"], "--flow-warps needs --flow"),
    (["--method", "block_matching", "--flow-warps", "1"], "--flow-warps needs --flow"),
    (["--flow", "--flow-warps", "5"], "--flow-warps must be from 0 to 4"),
    (["--flow", "--flow-warps", "x"], "--flow-warps must be from 0 to 4"),
])
def test_native_cli_usage_errors(nsc, tmp_path, extra, text):
    cli = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    assert os.path.exists(cli), "the native CLI is built with the library"
    out = str(tmp_path / "mid.png")
    r = subprocess.run([cli, "interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png"), out] + extra, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and text in r.stderr, (r.returncode, r.stderr)  # before anything is read: the frames do not exist
    assert not os.path.exists(out)
    assert "--flow-warps" in r.stderr  # the usage text names the flag
