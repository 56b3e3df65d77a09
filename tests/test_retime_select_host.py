"""Rate conversion with the select warp, the parts that need no GPU: the three entry points in the header and in the package's
binding (nus_interp_retime_select_device, nus_flow_estimate_both_device_stream, nus_flow_retime_select_device_stream), their
refusals -- each before any HIP call, so with the status and the text on a machine without a device --, the Python signatures and
defaults, the usage errors of both command-line tools, and the new kernels as the compiler builds them: no scratch, and no fewer
waves per SIMD than the multi-time select kernel of the same form."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "nuscaler_hip.h")

PROTOTYPES = {
    "nus_interp_retime_select_device":
        "int nus_interp_retime_select_device(nus_interp *h, const void *d_frames, size_t frame_stride, uint32_t n_frames, "
        "const void *d_flows_fwd, const void *d_flows_bwd, uint32_t w, uint32_t hgt, uint32_t num, uint32_t den, void *d_out, "
        "size_t out_frame_stride, void *stream);",
    "nus_flow_estimate_both_device_stream":
        "int nus_flow_estimate_both_device_stream(nus_flow *h, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t hgt, "
        "uint32_t levels, uint32_t coarse_iters, uint32_t refine_iters, float lambda, void *d_flows_fwd, void *d_flows_bwd, void *stream);",
    "nus_flow_retime_select_device_stream":
        "int nus_flow_retime_select_device_stream(nus_flow *h, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t hgt, "
        "uint32_t levels, uint32_t coarse_iters, uint32_t refine_iters, float lambda, uint32_t num, uint32_t den, int flow_format, "
        "void *d_flows_fwd, void *d_flows_bwd, void *d_out, size_t out_frame_stride, void *stream);",
}


def test_header_and_binding_carry_the_three_entry_points(nsc):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = nsc._capi.lib()
    vp, sz, u32, i, f = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_float
    kinds = {"*": vp, "size_t": sz, "uint32_t": u32, "int": i, "float": f}
    for name, proto in PROTOTYPES.items():
        m = re.search(r"^int " + name + r"\([^;]*\);", text, re.M)
        assert m, name
        assert " ".join(m.group(0).split()) == proto, name
        sig = [s for s in nsc._capi.SIGNATURES if s[0] == name]
        assert len(sig) == 1, name
        args = proto[proto.index("(") + 1:proto.rindex(")")].split(", ")
        want = [kinds["*"] if "*" in a else kinds[a.replace("const ", "").split()[0]] for a in args]
        assert sig[0][1] is i and list(sig[0][2]) == want, (name, sig[0][2])
        assert getattr(lib, name).argtypes == want


# ---- refusals: the status, a text that begins with the entry point's name, nothing touched ---------------------------------------------

W, H = 6, 4
FB = W * H * 4
PTR = 0x10000  # never dereferenced: every call below fails its checks
BAD_RATIOS = [((0, 1), "non-zero"), ((1, 0), "non-zero"), ((4097, 4096), "at most 4096"), ((1, 4097), "at most 4096"), ((9, 1), "at most 8")]


def _interp(nsc, lib, n_frames=3, num=5, den=2, frames=PTR, stride=FB, out=PTR, out_stride=0, fwd=PTR, bwd=PTR, w=W, h=H):
    it = nsc.WgpuFrameInterpolator()
    st = lib.nus_interp_retime_select_device(it._h, frames, stride, n_frames, fwd, bwd, w, h, num, den, out, out_stride, None)
    return st, it._err()


def _flow(nsc, lib, n_frames=3, num=5, den=2, frames=PTR, out=PTR, out_stride=0, fwd=None, bwd=None, fmt=0, w=W, h=H, bidirectional=False):
    fe = nsc.FlowEstimator(bidirectional=bidirectional)
    st = lib.nus_flow_retime_select_device_stream(fe._h, frames, n_frames, w, h, 1, 4, 2, ctypes.c_float(0.0004), num, den, fmt, fwd, bwd, out,
                                                  out_stride, None)
    return st, (lib.nus_flow_last_error(fe._h).decode() if fmt in (0, 1) else nsc._capi.last_error())


ENTRY = {"nus_interp_retime_select_device": _interp, "nus_flow_retime_select_device_stream": _flow}


@pytest.mark.parametrize("who", sorted(ENTRY))
def test_ratio_length_stride_and_alignment_errors_are_refused(nsc, who):
    lib = nsc._capi.lib()
    inv = nsc._capi.ERR_INVALID_ARGUMENT
    call = ENTRY[who]
    for (num, den), text in BAD_RATIOS:
        st, msg = call(nsc, lib, num=num, den=den)
        assert st == inv and msg.startswith(who + ":") and text in msg, (who, num, den, msg)
    for n in (0, 1):
        st, msg = call(nsc, lib, n_frames=n)
        assert st == inv and msg.startswith(who + ":") and "at least 2 frames" in msg, (who, n, msg)
    bad = [dict(out_stride=FB - 4), dict(out_stride=FB + 2), dict(out=PTR + 2), dict(frames=PTR + 1), dict(frames=None), dict(out=None),
           dict(w=0)]
    if who == "nus_interp_retime_select_device":
        bad += [dict(stride=FB - 4), dict(stride=FB + 2), dict(fwd=PTR + 4), dict(bwd=PTR + 4)]
    else:
        bad += [dict(out=PTR + 8), dict(fwd=PTR + 8), dict(bwd=PTR + 8), dict(fmt=2)]
    for kw in bad:
        st, msg = call(nsc, lib, **kw)
        assert st == inv and msg.startswith(who + ":"), (who, kw, st, msg)


def test_the_warp_entry_point_needs_both_flows(nsc):
    lib = nsc._capi.lib()
    for kw in (dict(fwd=None), dict(bwd=None), dict(fwd=None, bwd=None)):
        st, msg = _interp(nsc, lib, **kw)
        assert st == nsc._capi.ERR_INVALID_ARGUMENT and msg.startswith("nus_interp_retime_select_device:") and "both flows" in msg, (kw, msg)
    assert lib.nus_interp_retime_select_device(None, PTR, FB, 3, PTR, PTR, W, H, 5, 2, PTR, 0, None) == nsc._capi.ERR_INVALID_ARGUMENT
    assert nsc._capi.last_error() == "null handle"


def test_estimate_both_needs_both_buffers(nsc):
    lib = nsc._capi.lib()
    fe = nsc.FlowEstimator()
    for fwd, bwd in ((None, PTR), (PTR, None)):
        st = lib.nus_flow_estimate_both_device_stream(fe._h, PTR, 3, W, H, 1, 4, 2, ctypes.c_float(0.0004), fwd, bwd, None)
        msg = lib.nus_flow_last_error(fe._h).decode()
        assert st == nsc._capi.ERR_INVALID_ARGUMENT and msg.startswith("nus_flow_estimate_both_device_stream:"), (fwd, bwd, msg)
    with pytest.raises(ValueError, match="nus_flow_estimate_both_device_stream"):
        fe.estimate_both_device_stream(PTR, 3, W, H, PTR, 0)


def test_the_new_entry_points_do_not_look_at_the_setting(nsc):
    """With the bidirectional setting on, nus_flow_retime_device_stream still answers with its refusal; the select entry point's
    answers to a bad ratio are what they are with the setting off (it gets as far as its own checks)."""
    lib = nsc._capi.lib()
    st, msg = _flow(nsc, lib, num=9, den=1, bidirectional=True)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT and msg.startswith("nus_flow_retime_select_device_stream:") and "at most 8" in msg, msg
    fe = nsc.FlowEstimator(bidirectional=True)
    with pytest.raises(ValueError, match="bidirectional flow is not supported by rate conversion yet"):
        fe.retime_device_stream(PTR, 3, W, H, 5, 2, PTR)


def test_python_wrappers_signatures_and_defaults(nsc):
    from nu_scaler_amd import imagefile, retime, video
    from nu_scaler_amd.flow import FlowEstimator

    it = nsc.WgpuFrameInterpolator()
    p = list(inspect.signature(it.retime_select_device).parameters)
    assert p == ["d_frames", "frame_stride", "n_frames", "d_flows_fwd", "d_flows_bwd", "width", "height", "num", "den", "d_out",
                 "out_frame_stride", "stream"]
    p = inspect.signature(FlowEstimator.estimate_both_device_stream).parameters
    assert list(p)[1:] == ["d_frames", "n_frames", "width", "height", "d_flows_fwd", "d_flows_bwd", "stream"]
    p = inspect.signature(FlowEstimator.retime_select_device_stream).parameters
    assert list(p)[1:8] == ["d_frames", "n_frames", "width", "height", "num", "den", "d_out"]
    assert (p["d_flows_fwd"].default, p["d_flows_bwd"].default, p["out_frame_stride"].default, p["flow_format"].default) == (0, 0, 0, "f32")
    with pytest.raises(ValueError, match="nus_interp_retime_select_device"):
        it.retime_select_device(PTR, FB, 3, PTR, 0, W, H, 5, 2, PTR)
    with pytest.raises(ValueError, match="nus_interp_retime_select_device"):
        it.retime_select_device(PTR, FB, 3, PTR, PTR, W, H, 9, 1, PTR)
    with pytest.raises(ValueError, match="nus_flow_retime_select_device_stream"):
        FlowEstimator().retime_select_device_stream(PTR, 3, W, H, 9, 1, PTR)
    with pytest.raises(ValueError, match="flow_format"):
        FlowEstimator().retime_select_device_stream(PTR, 3, W, H, 5, 2, PTR, flow_format="f64")

    sel = inspect.signature(retime.retime_frames).parameters["select"]
    assert sel.default is False and sel.kind is inspect.Parameter.KEYWORD_ONLY
    frames = [bytes(FB)] * 3
    for kw in (dict(), dict(warp=it), dict(flow=FlowEstimator())):
        with pytest.raises(ValueError, match="select needs"):
            retime.retime_frames(frames, W, H, 24, 60, select=True, **kw)
    for fn in (imagefile.retime_image_files, video.convert_y4m, video.check_convert_args, video._Route.__init__):
        q = inspect.signature(fn).parameters["flow_bidirectional"]
        assert q.default is False, fn
    assert inspect.signature(video.check_convert_args).parameters["flow_bidirectional"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(video.check_convert_args).parameters)[:6] == ["fps_in", "fps_out", "multiplier", "method", "scale", "bidirectional"]


def test_check_convert_args_and_the_file_routes(nsc, tmp_path):
    from fractions import Fraction

    from nu_scaler_amd import imagefile, video

    assert video.check_convert_args(24, 60, None, "optical_flow", 1, False) == (Fraction(60), 5, 2)  # positional callers: as before
    assert video.check_convert_args(24, 60, None, "optical_flow", 1, False, flow_bidirectional=True) == (Fraction(60), 5, 2)
    for method in ("block_matching", "blend"):
        with pytest.raises(ValueError, match="^flow_bidirectional needs method optical_flow$"):
            video.check_convert_args(24, 60, None, method, 1, False, flow_bidirectional=True)
        with pytest.raises(ValueError, match="^flow_bidirectional needs method optical_flow$"):  # before anything is read
            imagefile.retime_image_files(str(tmp_path / "o_%d.png"), [str(tmp_path / "a.png"), str(tmp_path / "b.png")], 24, 60, method,
                                         flow_bidirectional=True)
    assert os.listdir(tmp_path) == []


# ---- both command-line tools ---------------------------------------------------------------------------------------------------------

ERROR_TEXT = "--flow-bidirectional needs --method optical_flow"  # the same in both tools


def test_python_cli_flags(nsc, capsys):
    from nu_scaler_amd import cli

    p = cli.build_parser()
    rt = ["retime", "--from", "24", "--to", "60", "OUT_%04d.png", "a.png", "b.png"]
    vd = ["video", "in.y4m", "out.y4m", "--to", "60"]
    for base in (rt, vd):
        assert p.parse_args(base).flow_bidirectional is False
        assert p.parse_args(base + ["--flow-bidirectional"]).flow_bidirectional is True
        for method in ("blend", "block_matching"):
            with pytest.raises(SystemExit) as e:  # usage errors: status 2 before anything is read
                cli.main(base + ["--method", method, "--flow-bidirectional"])
            assert e.value.code == 2
            assert ERROR_TEXT in capsys.readouterr().err
    for command in ("retime", "video"):
        with pytest.raises(SystemExit):
            cli.main([command, "--help"])
        assert "--flow-bidirectional" in capsys.readouterr().out  # the usage text names the flag


@pytest.mark.parametrize("tool", ["python", "native"])
def test_cli_usage_errors_give_status_2_and_touch_no_file(nsc, tmp_path, tool):
    argv = [sys.executable, "-m", "nu_scaler_amd.cli"] if tool == "python" else [os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")]
    if tool == "native":
        assert os.path.exists(argv[0]), "the native CLI is built with the library"
    env = dict(os.environ, PYTHONPATH=ROOT)
    tail = ["OUT_%04d.png", "missing0.png", "missing1.png"]
    for method in ("blend", "block_matching"):
        r = subprocess.run(argv + ["retime", "--from", "24", "--to", "60", "--method", method, "--flow-bidirectional"] + tail,
                           capture_output=True, text=True, cwd=tmp_path, env=env, timeout=120)
        assert r.returncode == 2 and ERROR_TEXT in r.stderr, (tool, method, r.returncode, r.stderr[-300:])
        if tool == "native":  # its usage text names the flag (the Python tool's: test_python_cli_flags)
            assert "[--flow-bidirectional] [--bidirectional]" in r.stderr
        assert os.listdir(tmp_path) == [], (tool, method)
    # a good command gets as far as reading its inputs, which do not exist
    r = subprocess.run(argv + ["retime", "--from", "24", "--to", "60", "--flow-bidirectional"] + tail, capture_output=True, text=True,
                       cwd=tmp_path, env=env, timeout=120)
    assert r.returncode == 1 and os.listdir(tmp_path) == [], (tool, r.returncode, r.stderr[-300:])
    if tool == "python":
        r = subprocess.run(argv + ["video", "in.y4m", "out.y4m", "--to", "60", "--method", "blend", "--flow-bidirectional"],
                           capture_output=True, text=True, cwd=tmp_path, env=env, timeout=120)
        assert r.returncode == 2 and ERROR_TEXT in r.stderr and os.listdir(tmp_path) == [], (r.returncode, r.stderr[-300:])
        r = subprocess.run(argv + ["video", "in.y4m", "out.y4m", "--to", "60", "--flow-bidirectional"], capture_output=True, text=True,
                           cwd=tmp_path, env=env, timeout=120)
        assert r.returncode == 1 and os.listdir(tmp_path) == [], (r.returncode, r.stderr[-300:])


# ---- the kernels as the compiler builds them -------------------------------------------------------------------------------------------


def _kernel_meta(asm, stem):
    out = {}
    for m in re.finditer(r"^\s+\.name:\s+(\S*" + stem + r"\S*)\s*$", asm, re.M):
        name = m.group(1)
        if name.endswith(".kd"):
            continue
        start = asm.rfind("- .agpr_count", 0, m.start())
        end = asm.find("- .agpr_count", m.end())
        out[name] = asm[start:end if end > 0 else len(asm)]
    return out


def _waves(meta):
    """Waves per SIMD of a gfx950 kernel from its register count: 512 registers per lane and SIMD, allocated in eights, at most 8 waves."""
    regs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))  # (the unified file's total: accumulation registers included)
    return min(8, 512 // (-(-regs // 8) * 8)), regs


@pytest.fixture(scope="module")
def units_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("asm")
    procs = {}
    for unit in ("nus_k_retime", "nus_k_warp_select"):  # side by side
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
               "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(d / (unit + ".s")),
               os.path.join(CSRC, unit + ".hip")]
        procs[unit] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for unit, p in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err
        out[unit] = (d / (unit + ".s")).read_text()
    return out


def test_retime_select_kernels_have_no_scratch_and_the_multi_time_kernels_occupancy(units_asm):
    new = _kernel_meta(units_asm["nus_k_retime"], "k_retime_flow_sel")
    old = _kernel_meta(units_asm["nus_k_warp_select"], "k_warp_blend_flow_selI")
    tile = {n: m for n, m in new.items() if "k_retime_flow_selI" in n}
    assert len(tile) == 8, sorted(new)  # MODE x HALF x (XV = 1, RV = 2 | XV = 2, RV = 1)
    assert sum("k_retime_flow_sel_tiny" in n for n in new) == 1
    for name, meta in new.items():
        for key in (".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size"):
            value = re.search(re.escape(key) + r":\s+(\d+)", meta)
            assert value and int(value.group(1)) == 0, (name, key, value and value.group(0))
    for name, meta in tile.items():
        # k_retime_flow_selILi<MODE>ELb<HALF>ELi<XV>ELi<RV>E...: its multi-time sibling is k_warp_blend_flow_selI<the same>ELb1E
        form = re.search(r"k_retime_flow_selI(Li\dELb\dELi\dELi\dE)", name).group(1)
        sibling = [m for n, m in old.items() if "k_warp_blend_flow_selI" + form + "Lb1E" in n]
        assert len(sibling) == 1, (name, sorted(old))
        (waves, regs), (waves_mt, regs_mt) = _waves(meta), _waves(sibling[0])
        print(f"{form}: retime {regs} VGPRs, {waves} waves per SIMD; multi-time {regs_mt} VGPRs, {waves_mt} waves per SIMD")
        assert waves >= waves_mt, (name, regs, regs_mt)
