"""The projection rounds of the dense-flow warp without a GPU (nus_interp_set_flow_project, nus_flow_set_project,
nus_flow_project): the exports, the header's prototypes and bound, the ABI version, the argument checks (before any HIP call, the
text begins with the entry point's name, the setting stays), the defaults, the Python wrappers' arguments and the flag of both
CLIs."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("nus_interp_set_flow_project", "nus_interp_flow_project", "nus_flow_set_project", "nus_flow_project_rounds", "nus_flow_project")


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


@pytest.fixture
def flow(lib):
    h = lib.nus_flow_create()
    assert h
    yield h
    lib.nus_flow_destroy(h)


@pytest.fixture
def interp(lib):
    h = lib.nus_interp_create(0)
    assert h
    yield h
    lib.nus_interp_destroy(h)


def test_exports_header_and_abi(nsc, lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in nsc._capi.SIGNATURES), name
    hdr = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    assert "#define NUS_FLOW_MAX_PROJECT 4\n" in hdr
    assert "int nus_interp_set_flow_project(nus_interp *h, uint32_t rounds);" in hdr
    assert "int nus_interp_flow_project(const nus_interp *h);" in hdr
    assert "int nus_flow_set_project(nus_flow *h, uint32_t rounds);" in hdr
    assert "int nus_flow_project_rounds(const nus_flow *h);" in hdr
    assert "int nus_flow_project(nus_flow *h, const float *flow_in, uint32_t w, uint32_t hgt, float t, uint32_t rounds, float *flow_out);" in hdr
    assert "BUILD-DEFINED" in hdr[hdr.index("Projection rounds of the dense-flow warp"):hdr.index("#define NUS_FLOW_MAX_PROJECT")]
    assert "#define NUS_ABI_VERSION 1\n" in hdr
    assert lib.nus_abi_version() == 1
    assert nsc._capi.FLOW_MAX_PROJECT == 4
    sys_rs = open(os.path.join(ROOT, "rust", "nu_scaler_hip-sys", "src", "lib.rs")).read()
    assert "pub const NUS_FLOW_MAX_PROJECT: c_int = 4;" in sys_rs
    assert "pub fn nus_interp_set_flow_project(h: *mut nus_interp, rounds: u32) -> c_int;" in sys_rs
    assert "pub fn nus_interp_flow_project(h: *const nus_interp) -> c_int;" in sys_rs
    assert "pub fn nus_flow_set_project(h: *mut nus_flow, rounds: u32) -> c_int;" in sys_rs
    assert "pub fn nus_flow_project_rounds(h: *const nus_flow) -> c_int;" in sys_rs
    assert ("pub fn nus_flow_project(h: *mut nus_flow, flow_in: *const f32, w: u32, hgt: u32, t: f32, rounds: u32, flow_out: *mut f32) "
            "-> c_int;") in sys_rs
    assert "nus_k_warp_project.hip" in open(os.path.join(ROOT, "nu_scaler_amd", "csrc", "Makefile")).read()


def test_defaults_and_argument_checks(nsc, lib, flow, interp):
    ok, inv = nsc._capi.OK, nsc._capi.ERR_INVALID_ARGUMENT
    for h, setter, getter, name, last in (
            (flow, lib.nus_flow_set_project, lib.nus_flow_project_rounds, "nus_flow_set_project", lib.nus_flow_last_error),
            (interp, lib.nus_interp_set_flow_project, lib.nus_interp_flow_project, "nus_interp_set_flow_project", lib.nus_interp_last_error)):
        assert getter(h) == 0
        assert setter(None, 1) == inv and nsc._capi.last_error() == "null handle"
        assert getter(None) == inv
        for rounds in (0, 1, 2, 3, 4, 0, 3):
            assert setter(h, rounds) == ok
            assert getter(h) == rounds
        for bad in (5, 6, 255, (1 << 32) - 1):
            assert setter(h, bad) == inv
            msg = last(h).decode()
            assert msg.startswith(name + ":"), msg
            assert nsc._capi.last_error() == msg
            assert getter(h) == 3  # left as it was
        assert setter(h, 0) == ok
    # nothing else moved, and no device was touched: no workspace
    assert lib.nus_flow_mode(flow) == 0 and lib.nus_flow_warps(flow) == 0 and lib.nus_flow_median_size(flow) == 0
    assert lib.nus_flow_workspace_bytes(flow) == 0
    assert lib.nus_interp_mode(interp) == 0
    assert lib.nus_flow_set_project(flow, 2) == ok and lib.nus_flow_set_warps(flow, 1) == ok and lib.nus_flow_set_median(flow, 5) == ok
    assert (lib.nus_flow_project_rounds(flow), lib.nus_flow_warps(flow), lib.nus_flow_median_size(flow)) == (2, 1, 5)  # independent


def test_primitive_checks_its_arguments_before_any_hip_call(nsc, lib, flow):
    inv = nsc._capi.ERR_INVALID_ARGUMENT
    buf = np.zeros(64, np.float32)
    out = np.zeros(64, np.float32)
    p, q = buf.ctypes.data, out.ctypes.data
    for bad in (5, 6, (1 << 32) - 1):
        assert lib.nus_flow_project(flow, p, 2, 2, 0.5, bad, q) == inv
        assert lib.nus_flow_last_error(flow).decode().startswith("nus_flow_project:")
    assert lib.nus_flow_project(flow, p, 2, 2, float("nan"), 1, q) == inv
    msg = lib.nus_flow_last_error(flow).decode()
    assert msg.startswith("nus_flow_project:") and "NaN" in msg, msg
    assert lib.nus_flow_project(flow, None, 2, 2, 0.5, 1, q) == inv
    assert lib.nus_flow_last_error(flow).decode().startswith("nus_flow_project:")
    assert lib.nus_flow_project(flow, p, 2, 2, 0.5, 1, None) == inv
    assert lib.nus_flow_project(flow, p, 0, 2, 0.5, 1, q) == inv
    assert lib.nus_flow_project(flow, p, 2, 0, 0.5, 1, q) == inv
    assert lib.nus_flow_project(None, p, 2, 2, 0.5, 1, q) == inv
    assert lib.nus_flow_workspace_bytes(flow) == 0  # refused before anything was reserved
    assert lib.nus_flow_project_rounds(flow) == 0  # the primitive is not the setting


def test_python_wrappers(nsc):
    from nu_scaler_amd.flow import FlowEstimator, check_project

    assert [check_project(n) for n in range(5)] == [0, 1, 2, 3, 4]
    assert check_project(np.int64(3)) == 3
    for bad in (-1, 5, 6, 2.0, 2.5, True, "2", None):
        with pytest.raises(ValueError, match="projection rounds"):
            check_project(bad)
    f = FlowEstimator()
    assert f.project == 0
    f.set_project(3)
    assert f.project == 3
    for bad in (-1, 5, 2.0, True, "3"):
        with pytest.raises(ValueError, match="projection rounds"):
            f.set_project(bad)
        assert f.project == 3  # a rejected call changes nothing
    f.set_project(0)
    assert f.project == 0
    assert FlowEstimator(project=2).project == 2
    every = FlowEstimator(warps=2, median=5, project=4)
    assert (every.warps, every.median_size, every.project) == (2, 5, 4)
    with pytest.raises(ValueError, match="projection rounds"):
        FlowEstimator(project=5)
    flow = np.zeros((4, 4, 2), np.float32)
    for bad in (-1, 5, True, 1.0):
        with pytest.raises(ValueError, match="projection rounds"):
            f.project_flow(flow, 0.5, bad)
    with pytest.raises(ValueError, match="flow"):
        f.project_flow(np.zeros((4, 4, 3), np.float32), 0.5, 1)
    with pytest.raises(ValueError, match="NaN"):
        f.project_flow(flow, float("nan"), 1)
    it = nsc.WgpuFrameInterpolator()
    assert it.flow_project == 0
    it.set_flow_project(4)
    assert it.flow_project == 4
    for bad in (-1, 5, 2.0, True):
        with pytest.raises(ValueError, match="projection rounds"):
            it.set_flow_project(bad)
        assert it.flow_project == 4
    it.set_flow_project(0)
    assert it.flow_project == 0 and it.mode == "exact"
    py = nsc.PyFrameInterpolator("optical_flow", flow_warps=1, flow_median=5, flow_project=3)
    assert py.name == "OpticalFlow" and py._warp.flow_project == 3 and py._flow.warps == 1 and py._flow.median_size == 5
    assert nsc.PyFrameInterpolator("optical_flow")._warp.flow_project == 0
    for method in ("block_matching", "simplified"):
        with pytest.raises(ValueError, match="flow_project"):
            nsc.PyFrameInterpolator(method, flow_project=1)
        assert nsc.PyFrameInterpolator(method, flow_project=0).name == "BlockMatching"
    for bad in (-1, 5, 7):
        with pytest.raises(ValueError, match="projection rounds"):
            nsc.PyFrameInterpolator("optical_flow", flow_project=bad)


def test_imagefile_and_step_motion_arguments(nsc, tmp_path):
    from nu_scaler_amd import imagefile
    from nu_scaler_amd.stream import FramePipeline

    assert inspect.signature(FramePipeline.step_motion).parameters["flow_project"].default == 0
    for fn in (imagefile.interpolate_image_files, imagefile.interpolate_image_files_multi):
        assert inspect.signature(fn).parameters["flow_project"].default == 0
    missing = str(tmp_path / "a.png")  # (the checks come before anything is read)
    with pytest.raises(ValueError, match="flow_project needs estimate_flow"):
        imagefile.interpolate_image_files(missing, missing, str(tmp_path / "o.png"), 0.5, False, flow_project=2)
    with pytest.raises(ValueError, match="projection rounds"):
        imagefile.interpolate_image_files(missing, missing, str(tmp_path / "o.png"), 0.5, True, flow_project=5)
    with pytest.raises(ValueError, match="flow_project needs estimate_flow"):
        imagefile.interpolate_image_files_multi(missing, missing, str(tmp_path / "o.png"), 2, False, flow_project=1)
    with pytest.raises(ValueError, match="projection rounds"):
        imagefile.interpolate_image_files_multi(missing, missing, str(tmp_path / "o.png"), 2, True, flow_project=-1)


def test_python_cli_flag(nsc, capsys):
    from nu_scaler_amd import cli

    p = cli.build_parser()
    base = ["interpolate", "a.png", "b.png", "out.png"]
    assert p.parse_args(base + ["--flow"]).flow_project is None
    assert p.parse_args(base + ["--flow", "--flow-project", "3"]).flow_project == 3
    assert p.parse_args(base + ["--flow", "--flow-warps", "2", "--flow-median", "5", "--flow-project", "2"]).flow_project == 2
    for argv, text in ((base + ["--flow-project", "2"], "--flow-project needs --flow"),
                       (base + ["--method", "block_matching", "--flow-project", "2"], "--flow-project needs --flow"),
                       (base + ["--flow", "--flow-project", "5"], "--flow-project must be from 0 to 4"),
                       (base + ["--flow", "--flow-project", "-1"], "--flow-project must be from 0 to 4")):
        with pytest.raises(SystemExit) as e:  # usage errors: status 2 before anything is read
            cli.main(argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err


@pytest.mark.parametrize("extra,text", [
    (["--flow-project", "2"], "--flow-project needs --flow"),
    (["--method", "block_matching", "--flow-project", "3"], "--flow-project needs --flow"),
    (["--flow", "--flow-project", "5"], "--flow-project must be from 0 to 4"),
    (["--flow", "--flow-project", "-1"], "--flow-project must be from 0 to 4"),
    (["--flow", "--flow-project", "x"], "--flow-project must be from 0 to 4"),
])
def test_native_cli_usage_errors(nsc, tmp_path, extra, text):
    cli = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    assert os.path.exists(cli), "the native CLI is built with the library"
    out = str(tmp_path / "mid.png")
    r = subprocess.run([cli, "interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png"), out] + extra, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and text in r.stderr, (r.returncode, r.stderr)  # before anything is read: the frames do not exist
    assert not os.path.exists(out)
    assert "--flow-project" in r.stderr  # the usage text names the flag
