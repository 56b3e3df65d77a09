"""The select warp and the estimator's bidirectional setting without a GPU (nus_interp_interpolate_select_device,
nus_interp_interpolate_select, nus_flow_set_bidirectional): the exports, the header's prototypes and the word BUILD-DEFINED, the
Rust declarations, the ABI version, the argument checks (before any HIP call, the text begins with the entry point's name, the
setting stays), the defaults, the Python wrappers' arguments, the flag of both CLIs, and the kernel unit as hipcc builds it for
gfx950: every instantiation there, none with a private segment or a spilled register."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("nus_interp_interpolate_select_device", "nus_interp_interpolate_select", "nus_flow_set_bidirectional", "nus_flow_bidirectional")
CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")


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
    hdr = " ".join(open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read().split())
    assert ("int nus_interp_interpolate_select_device(nus_interp *h, const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, "
            "const void *d_flow_fwd, const void *d_flow_bwd, uint32_t w, uint32_t hgt, const float *times, uint32_t n_times, void *d_out, "
            "size_t out_pair_stride, uint32_t n_pairs, void *stream);") in hdr
    assert ("int nus_interp_interpolate_select(nus_interp *h, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, "
            "const float *flow_fwd, const float *flow_bwd, uint32_t w, uint32_t hgt, const float *times, uint32_t n_times, uint8_t *out, "
            "size_t out_cap);") in hdr
    assert "int nus_flow_set_bidirectional(nus_flow *h, int enabled);" in hdr
    assert "int nus_flow_bidirectional(const nus_flow *h);" in hdr
    assert "BUILD-DEFINED" in hdr[hdr.index("The select warp"):hdr.index("int nus_interp_interpolate_select_device")]
    assert "BUILD-DEFINED" in hdr[hdr.index("Both flows of every pair"):hdr.index("int nus_flow_set_bidirectional")]
    assert "#define NUS_ABI_VERSION 1 " in hdr
    assert lib.nus_abi_version() == 1
    sys_rs = open(os.path.join(ROOT, "rust", "nu_scaler_hip-sys", "src", "lib.rs")).read()
    assert ("pub fn nus_interp_interpolate_select_device(h: *mut nus_interp, d_a: *const c_void, a_stride: usize, d_b: *const c_void, "
            "b_stride: usize, d_flow_fwd: *const c_void, d_flow_bwd: *const c_void, w: u32, hgt: u32, times: *const f32, n_times: u32, "
            "d_out: *mut c_void, out_pair_stride: usize, n_pairs: u32, stream: *mut c_void) -> c_int;") in sys_rs
    assert ("pub fn nus_interp_interpolate_select(h: *mut nus_interp, a: *const u8, a_len: usize, b: *const u8, b_len: usize, "
            "flow_fwd: *const f32, flow_bwd: *const f32, w: u32, hgt: u32, times: *const f32, n_times: u32, out: *mut u8, out_cap: usize) "
            "-> c_int;") in sys_rs
    assert "pub fn nus_flow_set_bidirectional(h: *mut nus_flow, enabled: c_int) -> c_int;" in sys_rs
    assert "pub fn nus_flow_bidirectional(h: *const nus_flow) -> c_int;" in sys_rs
    assert "nus_k_warp_select.hip" in open(os.path.join(CSRC, "Makefile")).read().split("KERNELS", 1)[1].split("\n", 1)[0]


def _times(*values):
    return (ctypes.c_float * len(values))(*values)


def test_select_device_checks_its_arguments_before_any_hip_call(nsc, lib, interp):
    ok, inv = nsc._capi.OK, nsc._capi.ERR_INVALID_ARGUMENT
    who = "nus_interp_interpolate_select_device:"
    assert lib.nus_interp_set_flow_project(interp, 3) == ok and lib.nus_interp_set_mode(interp, 1) == ok
    w, h = 6, 4
    fb = w * h * 4
    A, B, F, R, O = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # never dereferenced: every call below is refused first
    half = _times(0.5)

    def call(a=A, a_stride=fb, b=B, b_stride=fb, f=F, r=R, w_=w, h_=h, times=half, n=1, out=O, stride=0, pairs=1, handle=interp):
        return lib.nus_interp_interpolate_select_device(handle, a, a_stride, b, b_stride, f, r, w_, h_, times, n, out, stride, pairs, None)

    def refused(text=None, **kw):
        assert call(**kw) == inv, kw
        msg = lib.nus_interp_last_error(interp).decode()
        assert msg.startswith(who), msg
        assert nsc._capi.last_error() == msg
        if text:
            assert text in msg, msg
        assert lib.nus_interp_flow_project(interp) == 3 and lib.nus_interp_mode(interp) == 1  # the settings stay

    assert call(handle=None) == inv and nsc._capi.last_error() == "null handle"
    refused("flow", f=None)  # both flows are required
    refused("flow", r=None)
    refused("flow", f=None, r=None)
    refused("null", a=None)
    refused("null", b=None)
    refused("null", out=None)
    refused("n_times", n=0)
    refused("n_times", times=_times(*([0.5] * 8)), n=8)
    refused("times is null", times=None)
    refused("[0, 1]", times=_times(-0.25))
    refused("[0, 1]", times=_times(0.5, 1.5), n=2)
    refused("[0, 1]", times=_times(float("nan")))
    refused("aligned", a_stride=fb + 2)
    refused("aligned", b_stride=fb + 1)
    refused("aligned", f=F + 4)  # f32 flows: 8-byte cells
    refused("aligned", r=R + 4)
    refused("out_pair_stride", stride=fb - 4)
    refused("out_pair_stride", stride=2 * fb + 2, times=_times(0.25, 0.5), n=2)
    refused(w_=0)
    refused(h_=0)
    assert call(pairs=0) == ok  # nothing to do: NUS_OK, nothing launched
    assert lib.nus_interp_set_flow_format(interp, 1) == ok  # f16 flows: 4-byte cells
    refused("aligned", f=F + 2)
    refused("aligned", r=R + 2)


def test_select_host_checks_its_arguments_before_any_hip_call(nsc, lib, interp):
    inv, mismatch = nsc._capi.ERR_INVALID_ARGUMENT, nsc._capi.ERR_SIZE_MISMATCH
    who = "nus_interp_interpolate_select:"
    w, h = 6, 4
    fb = w * h * 4
    a, b, out = np.zeros(fb, np.uint8), np.zeros(fb, np.uint8), np.zeros(3 * fb, np.uint8)
    f, r = np.zeros(w * h * 2, np.float32), np.zeros(w * h * 2, np.float32)
    half = _times(0.5)

    def call(pa=a.ctypes.data, la=fb, pb=b.ctypes.data, lb=fb, pf=f.ctypes.data, pr=r.ctypes.data, times=half, n=1, po=out.ctypes.data,
             cap=out.nbytes, w_=w):
        return lib.nus_interp_interpolate_select(interp, pa, la, pb, lb, pf, pr, w_, h, times, n, po, cap)

    def refused(text, status=inv, **kw):
        assert call(**kw) == status, kw
        msg = lib.nus_interp_last_error(interp).decode()
        assert text in msg, msg
        if status == inv:
            assert msg.startswith(who), msg

    refused("flow", pf=None)
    refused("flow", pr=None)
    refused("null frame", pa=None)
    refused("null frame", po=None)
    refused("n_times", n=0)
    refused("n_times", times=_times(*([0.5] * 8)), n=8)
    refused("[0, 1]", times=_times(1.25))
    refused("[0, 1]", times=_times(float("nan")))
    refused("output capacity", times=_times(0.25, 0.5), n=2, cap=2 * fb - 1)
    refused("Expected", status=mismatch, la=fb - 4)  # the text of nus_interp_interpolate
    refused("", w_=0)
    assert not out.any()  # nothing ran


def test_bidirectional_setting_defaults_and_checks(nsc, lib, flow):
    ok, inv = nsc._capi.OK, nsc._capi.ERR_INVALID_ARGUMENT
    assert lib.nus_flow_bidirectional(flow) == 0  # off by default
    assert lib.nus_flow_set_bidirectional(None, 1) == inv and nsc._capi.last_error() == "null handle"
    assert lib.nus_flow_bidirectional(None) == inv
    for value in (1, 0, 1, 1):
        assert lib.nus_flow_set_bidirectional(flow, value) == ok
        assert lib.nus_flow_bidirectional(flow) == value
    for bad in (2, -1, 255):
        assert lib.nus_flow_set_bidirectional(flow, bad) == inv
        msg = lib.nus_flow_last_error(flow).decode()
        assert msg.startswith("nus_flow_set_bidirectional:"), msg
        assert lib.nus_flow_bidirectional(flow) == 1  # left as it was
    # rate conversion refuses the setting before it looks at anything else, and before any HIP call
    D = 0x10000
    st = lib.nus_flow_retime_device_stream(flow, D, 3, 6, 4, 3, 50, 10, 4e-4, 5, 2, 0, None, D, 0, None)
    msg = lib.nus_flow_last_error(flow).decode()
    assert st == inv and msg.startswith("nus_flow_retime_device_stream:"), msg
    assert msg.endswith("bidirectional flow is not supported by rate conversion yet"), msg
    assert lib.nus_flow_bidirectional(flow) == 1
    assert lib.nus_flow_workspace_bytes(flow) == 0  # nothing was reserved
    assert lib.nus_flow_set_bidirectional(flow, 0) == ok
    # off again: the same call gets past that check (and is refused for its null output instead)
    st = lib.nus_flow_retime_device_stream(flow, D, 3, 6, 4, 3, 50, 10, 4e-4, 5, 2, 0, None, None, 0, None)
    assert st == inv and "bidirectional" not in lib.nus_flow_last_error(flow).decode()
    # nothing else moved
    assert (lib.nus_flow_mode(flow), lib.nus_flow_warps(flow), lib.nus_flow_median_size(flow), lib.nus_flow_project_rounds(flow)) == (0, 0, 0, 0)


def test_python_wrappers(nsc):
    from nu_scaler_amd.flow import FlowEstimator

    f = FlowEstimator()
    assert f.bidirectional is False
    f.set_bidirectional(True)
    assert f.bidirectional is True
    for bad in (2, -1, "yes", None, 0.5):
        with pytest.raises(ValueError, match="bidirectional"):
            f.set_bidirectional(bad)
        assert f.bidirectional is True  # a rejected call changes nothing
    with pytest.raises(ValueError, match="bidirectional flow is not supported by rate conversion yet"):
        f.retime_device_stream(0x10000, 3, 6, 4, 5, 2, 0x20000)
    f.set_bidirectional(False)
    assert f.bidirectional is False
    assert FlowEstimator(bidirectional=True).bidirectional is True
    assert inspect.signature(FlowEstimator.__init__).parameters["bidirectional"].default is False
    every = FlowEstimator(warps=2, median=5, project=4, bidirectional=True)
    assert (every.warps, every.median_size, every.project, every.bidirectional) == (2, 5, 4, True)

    it = nsc.WgpuFrameInterpolator()
    sig = inspect.signature(it.interpolate_select_py)
    assert list(sig.parameters)[:6] == ["frame_a_bytes", "frame_b_bytes", "width", "height", "flow_fwd", "flow_bwd"]
    assert sig.parameters["time_t"].default == 0.5 and sig.parameters["time_t"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(it.interpolate_select_multi_py)
    assert sig.parameters["times"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["multiplier"].default is None
    assert "d_flow_bwd" in inspect.signature(it.interpolate_select_device).parameters
    w, h = 6, 4
    a = b = bytes(w * h * 4)
    flow = np.zeros((h, w, 2), np.float32)
    for kw in ({}, {"times": [0.5], "multiplier": 2}, {"times": []}, {"times": [0.5] * 8}, {"times": [1.5]}, {"times": [float("nan")]},
               {"multiplier": 9}):
        with pytest.raises(ValueError):
            it.interpolate_select_multi_py(a, b, w, h, flow, flow, **kw)
    with pytest.raises(ValueError, match="flow_bwd"):
        it.interpolate_select_py(a, b, w, h, flow, None)
    with pytest.raises(ValueError, match="flow_fwd"):
        it.interpolate_select_py(a, b, w, h, None, flow)
    with pytest.raises(ValueError, match="flow_bwd"):
        it.interpolate_select_py(a, b, w, h, flow, flow[:2])
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        it.interpolate_select_py(a, b, w, h, flow, flow, time_t=2.0)
    with pytest.raises(ValueError, match="nus_interp_interpolate_select_device"):
        it.interpolate_select_device(0x10000, 96, 0x20000, 96, 0x30000, 0, w, h, [0.5], 0x50000)

    py = nsc.PyFrameInterpolator("optical_flow", flow_warps=1, flow_median=5, flow_project=3, flow_bidirectional=True)
    assert py.name == "OpticalFlow" and py._flow.bidirectional is True and py._warp.flow_project == 3
    assert nsc.PyFrameInterpolator("optical_flow")._flow.bidirectional is False
    for method in ("block_matching", "simplified"):
        with pytest.raises(ValueError, match="flow_bidirectional"):
            nsc.PyFrameInterpolator(method, flow_bidirectional=True)
        assert nsc.PyFrameInterpolator(method, bidirectional=True).name == "BlockMatching"  # the block matcher's own, a different thing
    with pytest.raises(ValueError, match="forward-backward"):
        nsc.PyFrameInterpolator("optical_flow", bidirectional=True)
    py.initialize(w, h)
    with pytest.raises(ValueError, match="bidirectional flow is not supported by rate conversion yet"):
        py.retime([a, a, a], 24, 60)


def test_imagefile_arguments(nsc, tmp_path):
    from nu_scaler_amd import imagefile

    for fn in (imagefile.interpolate_image_files, imagefile.interpolate_image_files_multi):
        assert inspect.signature(fn).parameters["flow_bidirectional"].default is False
    missing = str(tmp_path / "a.png")  # (the checks come before anything is read)
    with pytest.raises(ValueError, match="flow_bidirectional needs estimate_flow"):
        imagefile.interpolate_image_files(missing, missing, str(tmp_path / "o.png"), 0.5, False, flow_bidirectional=True)
    with pytest.raises(ValueError, match="flow_bidirectional needs estimate_flow"):
        imagefile.interpolate_image_files_multi(missing, missing, str(tmp_path / "o.png"), 2, False, flow_bidirectional=True)


ERROR_TEXT = "--flow-bidirectional needs --flow"  # the same in both tools


def test_python_cli_flag(nsc, capsys):
    from nu_scaler_amd import cli

    p = cli.build_parser()
    base = ["interpolate", "a.png", "b.png", "out.png"]
    assert p.parse_args(base + ["--flow"]).flow_bidirectional is False
    assert p.parse_args(base + ["--flow", "--flow-bidirectional"]).flow_bidirectional is True
    args = p.parse_args(base + ["--flow", "--flow-warps", "2", "--flow-median", "5", "--flow-project", "3", "--flow-bidirectional",
                                "--multiplier", "4", "--scene-detect"])
    assert (args.flow_bidirectional, args.flow_warps, args.flow_median, args.flow_project, args.multiplier, args.scene_detect) == (
        True, 2, 5, 3, 4, True)
    for argv in (base + ["--flow-bidirectional"], base + ["--method", "block_matching", "--flow-bidirectional"]):
        with pytest.raises(SystemExit) as e:  # usage errors: status 2 before anything is read
            cli.main(argv)
        assert e.value.code == 2
        assert ERROR_TEXT in capsys.readouterr().err


@pytest.mark.parametrize("extra", [["--flow-bidirectional"], ["--method", "block_matching", "--flow-bidirectional"],
                                   ["--multiplier", "3", "--flow-bidirectional"]])
def test_native_cli_usage_errors(nsc, tmp_path, extra):
    cli = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    assert os.path.exists(cli), "the native CLI is built with the library"
    out = str(tmp_path / "mid.png")
    r = subprocess.run([cli, "interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png"), out] + extra, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and ERROR_TEXT in r.stderr, (r.returncode, r.stderr)  # before anything is read: the frames do not exist
    assert not os.path.exists(out)
    assert "[--flow-bidirectional]" in r.stderr  # the usage text names the flag


# ---- the kernel unit as the compiler builds it ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def select_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("asm") / "nus_k_warp_select.s"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
           "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out),
           os.path.join(CSRC, "nus_k_warp_select.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return out.read_text()


def test_every_instantiation_is_there_and_none_spills(select_asm):
    kernels = {}
    for m in re.finditer(r"^\s+\.name:\s+(\S*k_warp_blend_flow_sel\S*)\s*$", select_asm, re.M):
        name = m.group(1)
        if name.endswith(".kd"):
            continue
        start = select_asm.rfind("- .agpr_count", 0, m.start())
        end = select_asm.find("- .agpr_count", m.end())
        kernels[name] = select_asm[start:end if end > 0 else len(select_asm)]
    tile = [n for n in kernels if "k_warp_blend_flow_selI" in n]
    assert len(tile) == 16, sorted(kernels)  # MODE x HALF x (XV = 2, 1) x MT
    assert sum("k_warp_blend_flow_sel_tiny" in n for n in kernels) == 2  # MT
    for name, meta in kernels.items():
        for key in (".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"):
            value = re.search(re.escape(key) + r":\s+(\d+)", meta)
            assert value and int(value.group(1)) == 0, (name, key, value and value.group(0))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
        print(f"{name}: {vgprs} VGPRs")
        assert vgprs <= 96, name  # five waves per SIMD at the least
