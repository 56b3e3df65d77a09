"""Rate conversion with the select warp behind the estimator, on the MI355X.

  nus_flow_estimate_both_device_stream   the forward flows are nus_flow_estimate_device_stream's bytes; in EXACT mode backward
        plane k is nus_flow_estimate_device(frame k+1, frame k); in every mode the two outputs, fed to the select warp in FMA mode,
        give the frames of nus_flow_interpolate_multi_device_stream on a handle with the bidirectional setting on -- which ties the
        backward flows handed out to the ones the setting keeps in its workspace, FAST included.
  nus_flow_retime_select_device_stream   equals the entry point above followed by nus_interp_retime_select_device in FMA mode,
        byte for byte: both flow formats, warps, median and projection set, chunks of 1, 2 and all pairs, with and without the
        caller's flow buffers, after the workspace was filled with 0xFF; at most 28 bytes per pixel and pair of a chunk more
        workspace than nus_flow_retime_device_stream; scene detection behind it; a handle that ran them is a fresh handle to the
        old entry points.
  above the library   retime_frames(select=True), retime_image_files(flow_bidirectional=True), both command-line tools and
        convert_y4m(flow_bidirectional=True).

At 67 x 45 and at 66 x 44 (the pixel-pair kernels).  Every device output comes from conftest.guarded."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _flow_warp64 as W64
import _retime
from conftest import ROOT, guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

P = W64.PARAMS
TABLE = (P["levels"], P["coarse_iters"], P["refine_iters"])
SIZES = [(67, 45), (66, 44)]
MODES = [("fast", 1), ("exact", 0), ("exact", 1)]  # the FAST batch path, the EXACT pair-by-pair path, the EXACT batch path
TIMES3 = [float(np.float32(0.25)), 0.5, float(np.float32(0.7))]
CHUNK_ENV = "NUS_FLOW_MAX_CHUNK_PAIRS"
POISON = 0x3C
ROUNDS = 2


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _lattice(w, h, n):
    frames = W64.lattice_frames(w, h, n)
    frames.setflags(write=False)
    return frames


def _estimator(nsc, mode, tiled, bidirectional=False, warps=1, median=3, project=ROUNDS):
    fe = nsc.FlowEstimator(TABLE[0], TABLE[1], TABLE[2], P["lam"], warps=warps, median=median, project=project, bidirectional=bidirectional)
    fe.set_mode(mode)
    fe.set_tiled(tiled)
    return fe


def _warp(nsc, ffmt="f32", mode="fma", rounds=ROUNDS):
    it = nsc.WgpuFrameInterpolator()
    it.set_mode(mode)
    it.set_flow_format(ffmt)
    it.set_flow_project(rounds)
    return it


def _nan_flows(n_pairs, w, h, ffmt="f32"):
    import torch

    return guarded.full((n_pairs, h, w, 2), float("nan"), dtype=torch.float32 if ffmt == "f32" else torch.float16, device="cuda:0")


def _both(fe, d, n, w, h):
    """nus_flow_estimate_both_device_stream -> (forward, backward), each (n - 1, h, w, 2) float32 on the host."""
    fwd, bwd = _nan_flows(n - 1, w, h), _nan_flows(n - 1, w, h)
    fe.estimate_both_device_stream(d.data_ptr(), n, w, h, fwd.data_ptr(), bwd.data_ptr(), _stream())
    return fetch(fwd), fetch(bwd)


def _out(n_out, w, h):
    import torch

    return guarded.full((n_out, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")


def _assert_bytes(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint8), want.view(np.uint8)):
        diff = (got.view(np.uint8) != want.view(np.uint8))
        raise AssertionError(f"{tag}: {int(diff.sum())} of {diff.size} bytes differ, first at {tuple(int(v) for v in np.argwhere(diff)[0])}")


@pytest.fixture
def chunk_env():
    """set(value or None) for NUS_FLOW_MAX_CHUNK_PAIRS; whatever the process had comes back afterwards."""
    old = os.environ.pop(CHUNK_ENV, None)

    def set_(value):
        os.environ.pop(CHUNK_ENV, None)
        if value is not None:
            os.environ[CHUNK_ENV] = str(value)

    yield set_
    os.environ.pop(CHUNK_ENV, None)
    if old is not None:
        os.environ[CHUNK_ENV] = old


# ---- 1. both flows out of the estimator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("mode,tiled", MODES)
def test_estimate_both_hands_out_the_flows_the_setting_uses(nsc, chunk_env, mode, tiled, w, h):
    import torch

    chunk_env(None)
    n = 4
    frames = _lattice(w, h, n)
    d = put(frames, "cuda:0")
    fb, plane = w * h * 4, w * h * 8
    s = _stream()
    fwd, bwd = _both(_estimator(nsc, mode, tiled), d, n, w, h)
    assert not np.isnan(fwd).any() and not np.isnan(bwd).any()
    assert float(np.abs(fwd).max()) > 1.5 and float(np.abs(fwd + bwd).max()) > 0.25  # motion, and the two estimates are not mirror images
    plain = _nan_flows(n - 1, w, h)
    _estimator(nsc, mode, tiled).estimate_device_stream(d.data_ptr(), n, w, h, plain.data_ptr(), s)
    _assert_bytes(fwd, fetch(plain), ("forward flows", mode, tiled, w, h))
    # the bidirectional setting changes nothing: the entry point does not look at it
    on = _both(_estimator(nsc, mode, tiled, True), d, n, w, h)
    _assert_bytes(on[0], fwd, ("forward flows, setting on", mode, tiled)), _assert_bytes(on[1], bwd, ("backward flows, setting on", mode, tiled))
    if mode == "exact":
        pair = _nan_flows(n - 1, w, h)
        est = _estimator(nsc, mode, tiled)
        for k in range(n - 1):
            est.estimate_device(d.data_ptr() + (k + 1) * fb, d.data_ptr() + k * fb, w, h, pair.data_ptr() + k * plane, s)
        _assert_bytes(bwd, fetch(pair), ("backward plane k against nus_flow_estimate_device(k + 1, k)", tiled, w, h))
    for ffmt in ("f32", "f16"):
        cast = (lambda f: f) if ffmt == "f32" else (lambda f: f.astype(np.float16))
        d_fwd, d_bwd = put(cast(fwd)), put(cast(bwd))
        want = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
        _warp(nsc, ffmt).interpolate_select_device(d.data_ptr(), fb, d.data_ptr() + fb, fb, d_fwd.data_ptr(), d_bwd.data_ptr(), w, h, TIMES3,
                                                   want.data_ptr(), 0, n - 1, s)
        mid = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
        _estimator(nsc, mode, tiled, True).interpolate_multi_device_stream(d.data_ptr(), n, w, h, TIMES3, mid.data_ptr(), 0, 0, s, flow_format=ffmt)
        _assert_bytes(fetch(mid), fetch(want), ("the setting's frames from the flows handed out", mode, tiled, ffmt, w, h))
    assert np.array_equal(fetch(d), frames)  # the frames are inputs


# ---- 2. the fused route ------------------------------------------------------------------------------------------------------------------
def _fused(fe, d, n, w, h, num, den, ffmt, with_fwd, with_bwd):
    """nus_flow_retime_select_device_stream -> (frames, forward buffer, backward buffer); a buffer not handed in keeps its NaNs."""
    out = _out(_retime.count(n, num, den), w, h)
    fwd, bwd = _nan_flows(n - 1, w, h, ffmt), _nan_flows(n - 1, w, h, ffmt)
    fe.retime_select_device_stream(d.data_ptr(), n, w, h, num, den, out.data_ptr(), fwd.data_ptr() if with_fwd else 0,
                                   bwd.data_ptr() if with_bwd else 0, 0, _stream(), flow_format=ffmt)
    return fetch(out), fetch(fwd), fetch(bwd)


@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("mode,tiled", MODES)
def test_fused_route_equals_estimate_both_then_the_select_conversion(nsc, monkeypatch, chunk_env, mode, tiled, w, h, ffmt):
    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    n = 5
    frames = _lattice(w, h, n)
    d = put(frames, "cuda:0")
    fb = w * h * 4
    s = _stream()
    cast = (lambda f: f) if ffmt == "f32" else (lambda f: f.astype(np.float16))
    it = _warp(nsc, ffmt)
    for chunk, ratios in ((1, [(5, 2)]), (2, [(5, 2)]), (None, [(5, 2), (12, 5), (2, 5)])):
        chunk_env(chunk)  # (the pair-by-pair path has no chunks: the same route three times)
        fwd, bwd = (cast(f) for f in _both(_estimator(nsc, mode, tiled), d, n, w, h))
        d_fwd, d_bwd = put(fwd), put(bwd)
        fe = _estimator(nsc, mode, tiled)
        for num, den in ratios:
            tag = (mode, tiled, w, h, ffmt, chunk, num, den)
            n_out = _retime.count(n, num, den)
            want = _out(n_out, w, h)
            it.retime_select_device(d.data_ptr(), fb, n, d_fwd.data_ptr(), d_bwd.data_ptr(), w, h, num, den, want.data_ptr(), 0, s)
            want = fetch(want)
            got, f_out, b_out = _fused(fe, d, n, w, h, num, den, ffmt, True, True)
            _assert_bytes(got, want, (tag, "frames"))
            _assert_bytes(f_out, fwd, (tag, "d_flows_fwd")), _assert_bytes(b_out, bwd, (tag, "d_flows_bwd"))
            for with_fwd, with_bwd in ((False, False), (True, False), (False, True)):
                got, f_out, b_out = _fused(fe, d, n, w, h, num, den, ffmt, with_fwd, with_bwd)
                _assert_bytes(got, want, (tag, with_fwd, with_bwd, "frames"))
                for given, buf, ref in ((with_fwd, f_out, fwd), (with_bwd, b_out, bwd)):
                    if given:
                        _assert_bytes(buf, ref, (tag, with_fwd, with_bwd, "a flow buffer"))
                    else:
                        assert np.isnan(buf.astype(np.float32)).all(), (tag, with_fwd, with_bwd, "a buffer that was not handed in was written")
            fe._fill_workspace(0xFF, s)
            _assert_bytes(_fused(fe, d, n, w, h, num, den, ffmt, False, False)[0], want, (tag, "after a fill with 0xff"))
            if (num, den) != (2, 5):  # the backward flow does something here: the plain conversion's frames differ
                plain = _out(n_out, w, h)
                _estimator(nsc, mode, tiled).retime_device_stream(d.data_ptr(), n, w, h, num, den, plain.data_ptr(), 0, 0, s, flow_format=ffmt)
                assert not np.array_equal(fetch(plain), want), (tag, "a route that ignores the backward flow would pass")
            for j, (k, r, t) in enumerate(_retime.schedule(n, num, den)):
                if r == 0:
                    assert np.array_equal(want[j], frames[k]), (tag, j, "a real-frame output is not the input frame")
    assert np.array_equal(fetch(d), frames)


# ---- 3. what it costs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tiled,w,h,n,ffmt,flows,chunk", [
    ("exact", 1, 66, 44, 4, "f32", False, None), ("exact", 1, 66, 44, 4, "f32", True, None), ("exact", 3, 67, 45, 5, "f16", False, None),
    ("exact", 2, 67, 45, 5, "f16", True, None), ("exact", 0, 66, 44, 4, "f32", False, None), ("exact", 0, 66, 44, 4, "f16", True, None),
    ("fast", 3, 66, 44, 4, "f16", False, None), ("exact", 1, 67, 45, 6, "f32", False, 2)])
def test_at_most_28_bytes_per_pixel_and_pair_more_than_the_plain_conversion(nsc, chunk_env, mode, tiled, w, h, n, ffmt, flows, chunk):
    """include/nuscaler_hip.h: at most 28 B per pixel and pair of a chunk more than nus_flow_retime_device_stream reserves for the
    same call -- the forward flows kept from the backward solve and the backward flows (8 B each where the caller gives no buffer)
    and the backward solve's coefficients (12 B); the pair-by-pair path holds one pair's.  DeviceBuffer::reserve allocates exactly
    the bytes it is asked for, so the bound is the product itself."""
    import torch

    chunk_env(chunk)
    d = put(_lattice(w, h, n), "cuda:0")
    held = {}
    for select in (False, True):
        fe = _estimator(nsc, mode, tiled)
        out = _out(_retime.count(n, 5, 2), w, h)
        fwd, bwd = _nan_flows(n - 1, w, h, ffmt), _nan_flows(n - 1, w, h, ffmt)
        if select:
            fe.retime_select_device_stream(d.data_ptr(), n, w, h, 5, 2, out.data_ptr(), fwd.data_ptr() if flows else 0,
                                           bwd.data_ptr() if flows else 0, 0, _stream(), flow_format=ffmt)
        else:
            fe.retime_device_stream(d.data_ptr(), n, w, h, 5, 2, out.data_ptr(), fwd.data_ptr() if flows else 0, 0, _stream(), flow_format=ffmt)
        torch.cuda.synchronize()
        held[select] = fe.workspace_bytes
    chunk_pairs = 1 if (mode, tiled) == ("exact", 0) else min(n - 1, chunk or n - 1)
    bound = 28 * w * h * chunk_pairs
    print(f"{mode} {tiled} {w}x{h} n {n} {ffmt} flows {flows} chunk {chunk}: plain {held[False]} B, select {held[True]} B: "
          f"{held[True] - held[False]} B more, bound {bound} B")
    assert 0 < held[True] - held[False] <= bound, (held, bound)


# ---- 4. scene detection behind it ----------------------------------------------------------------------------------------------------------
def _cut_stream(lattice):
    frames = np.array(lattice)
    frames[3:] = frames[3:][..., ::-1, :] // 4  # from frame 3 on another, dark scene: pair (2, 3) is the one hard cut
    frames[..., 3] = 255
    return frames


@pytest.mark.parametrize("w,h", SIZES)
def test_scene_detection_repeats_the_nearer_frame_on_the_cut_pair_only(nsc, chunk_env, w, h):
    import _scenecut as sc

    chunk_env(None)
    n = 5
    frames = _cut_stream(_lattice(w, h, n))
    assert [bool(sc.is_cut(*sc.measures(frames[k], frames[k + 1]), w, h)) for k in range(n - 1)] == [False, False, True, False]
    d = put(frames, "cuda:0")
    fe = _estimator(nsc, "exact", 1)
    for num, den in [(5, 2), (12, 5), (2, 5)]:
        off = _fused(fe, d, n, w, h, num, den, "f32", False, False)[0]
        fe.set_scene_detect(True)
        try:
            on = _fused(fe, d, n, w, h, num, den, "f32", False, False)[0]
        finally:
            fe.set_scene_detect(False)
        touched = 0
        for j, (k, r, t) in enumerate(_retime.schedule(n, num, den)):
            if r != 0 and k == 2:
                assert np.array_equal(on[j], frames[2] if float(t) < 0.5 else frames[3]), (w, h, num, den, j)
                assert not np.array_equal(on[j], off[j])
                touched += 1
            else:
                assert np.array_equal(on[j], off[j]), (w, h, num, den, j)
        assert touched or (num, den) == (2, 5)


# ---- 5. the old entry points afterwards --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tiled", MODES)
def test_a_handle_that_ran_the_new_entry_points_is_a_fresh_handle_to_the_old_ones(nsc, chunk_env, mode, tiled):
    import torch

    chunk_env(None)
    w, h, n = 67, 45, 4
    d = put(_lattice(w, h, n), "cuda:0")
    s = _stream()
    out = {}
    for name in ("used", "fresh"):
        fe = _estimator(nsc, mode, tiled)
        if name == "used":
            _both(fe, d, n, w, h)
            _fused(fe, d, n, w, h, 5, 2, "f32", True, True), _fused(fe, d, n, w, h, 12, 5, "f16", False, False)
        assert fe.bidirectional is False
        got = []
        for ffmt in ("f32", "f16"):
            mid = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
            flows = _nan_flows(n - 1, w, h, ffmt)
            fe.interpolate_multi_device_stream(d.data_ptr(), n, w, h, TIMES3, mid.data_ptr(), flows.data_ptr(), 0, s, flow_format=ffmt)
            conv = _out(_retime.count(n, 5, 2), w, h)
            flows2 = _nan_flows(n - 1, w, h, ffmt)
            fe.retime_device_stream(d.data_ptr(), n, w, h, 5, 2, conv.data_ptr(), flows2.data_ptr(), 0, s, flow_format=ffmt)
            got += [fetch(mid), fetch(flows), fetch(conv), fetch(flows2)]
        out[name] = got
    for x, y in zip(out["used"], out["fresh"]):
        _assert_bytes(x, y, (mode, tiled))


# ---- 6. the package's routes and both command-line tools ---------------------------------------------------------------------------------------
def test_retime_frames_with_select_returns_the_device_bytes(nsc, chunk_env):
    from nu_scaler_amd.retime import retime_frames

    chunk_env(None)
    w, h, n = 67, 45, 4
    frames = _lattice(w, h, n)
    d = put(frames, "cuda:0")
    fb = w * h * 4
    fe, it = nsc.FlowEstimator(), nsc.WgpuFrameInterpolator()
    got = retime_frames([f.tobytes() for f in frames], w, h, 24, 60, warp=it, flow=fe, select=True)
    fwd, bwd = _both(nsc.FlowEstimator(), d, n, w, h)
    d_fwd, d_bwd = put(fwd), put(bwd)
    want = _out(_retime.count(n, 5, 2), w, h)
    nsc.WgpuFrameInterpolator().retime_select_device(d.data_ptr(), fb, n, d_fwd.data_ptr(), d_bwd.data_ptr(), w, h, 5, 2, want.data_ptr(), 0,
                                                     _stream())
    want = fetch(want)
    assert len(got) == len(want) and all(g == w_.tobytes() for g, w_ in zip(got, want))
    plain = retime_frames([f.tobytes() for f in frames], w, h, 24, 60, warp=it, flow=fe)
    assert plain != got and plain[0] == got[0]  # select does something; a real frame is a real frame
    assert retime_frames([f.tobytes() for f in frames], w, h, 24, 60, warp=it, flow=fe, select=False) == plain


def _run_cli(argv, args, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(argv + ["retime"] + args, capture_output=True, text=True, cwd=tmp_path, env=env, timeout=300)
    assert r.returncode == 0, (argv, args, r.stdout, r.stderr)
    return r.stdout.split()


def test_image_files_and_both_clis_write_the_same_pngs(nsc, chunk_env, tmp_path):
    """Three inputs at 24 -> 60: retime_image_files(flow_bidirectional=True), `python -m nu_scaler_amd.cli retime
    --flow-bidirectional` (the device-resident conversion) and the native tool (per pair: the estimate both ways and
    nus_interp_interpolate_select at the schedule's times) write the same PNGs, the frames of retime_frames(select=True)."""
    from _png import read_png
    from nu_scaler_amd.imagefile import retime_image_files, write_png
    from nu_scaler_amd.retime import retime_frames

    chunk_env(None)
    w, h, n = 67, 45, 3
    frames = _lattice(w, h, n)
    inputs = []
    for k, f in enumerate(frames):
        inputs.append(str(tmp_path / f"in{k}.png"))
        write_png(inputs[-1], w, h, f.tobytes())
    want = retime_frames([f.tobytes() for f in frames], w, h, 24, 60, warp=nsc.WgpuFrameInterpolator(), flow=nsc.FlowEstimator(), select=True)
    sched = _retime.schedule(n, 5, 2)
    assert len(want) == len(sched) == 6
    lib = retime_image_files(str(tmp_path / "lib_%04d.png"), inputs, 24, 60, "optical_flow", flow_bidirectional=True)
    assert lib == [str(tmp_path / f"lib_{j:04d}.png") for j in range(6)]
    py = _run_cli([sys.executable, "-m", "nu_scaler_amd.cli"], ["--from", "24", "--to", "60", "--flow-bidirectional", "py_%04d.png"] + inputs, tmp_path)
    assert py == [f"py_{j:04d}.png" for j in range(6)]
    legs = {"package": lib, "python tool": [str(tmp_path / p) for p in py]}
    native = os.path.join(os.path.dirname(os.path.dirname(nsc._capi.LIB_PATH)), "bin", "nu_scaler_cli")
    if os.path.exists(native):
        nat = _run_cli([native], ["--from", "24", "--to", "60", "--flow-bidirectional", "nat_%04d.png"] + inputs, tmp_path)
        assert nat == [f"nat_{j:04d}.png" for j in range(6)]
        legs["native tool"] = [str(tmp_path / p) for p in nat]
    for leg, paths in legs.items():
        for j, path in enumerate(paths):
            assert read_png(path).tobytes() == want[j], (leg, j, sched[j])
    plain = retime_image_files(str(tmp_path / "plain_%04d.png"), inputs, 24, 60, "optical_flow")
    assert any(read_png(p).tobytes() != want[j] for j, p in enumerate(plain)), "the flag does something"
    if "native tool" not in legs:
        pytest.skip("the native tool is not built here: the package and the Python tool agree")


# ---- 7. Y4M video --------------------------------------------------------------------------------------------------------------------------------
def test_convert_y4m_with_the_select_warp(nsc, chunk_env, tmp_path):
    """tests/test_gpu_video.py's clip at 24 -> 60 with flow_bidirectional: a window of 3 frames and one window give identical
    files, and every frame equals to_rgba -> retime_frames(select=True) over the whole clip -> to_yuv."""
    import test_gpu_video as V
    from nu_scaler_amd.retime import retime_frames
    from nu_scaler_amd.y4m import Y4MReader

    chunk_env(None)
    frames = V._clip()
    src = V._write_clip(tmp_path / "in.y4m", b"YUV4MPEG2 W64 H48 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL", frames)
    outs = {}
    for win in (3, V.N):
        out = str(tmp_path / f"out{win}.y4m")
        r = nsc.convert_y4m(src, out, fps_out=60, window_frames=win, matrix="bt601", flow_bidirectional=True)
        assert (r["frames_in"], r["frames_out"], r["windows"]) == (V.N, 26, {3: 5, V.N: 1}[win])
        outs[win] = open(out, "rb").read()
    assert outs[3] == outs[V.N]
    with Y4MReader(str(tmp_path / "out3.y4m")) as rd:
        got = list(rd)
    fmt = nsc.YuvFormat("bt601", "full", "left", "bilinear")
    rgba = [nsc.yuv.to_rgba(f, V.W, V.H, fmt) for f in frames]
    conv = retime_frames(rgba, V.W, V.H, 24, 60, warp=nsc.WgpuFrameInterpolator(), flow=nsc.FlowEstimator(), select=True)
    want = [nsc.yuv.to_yuv(o, V.W, V.H, fmt) for o in conv]
    assert len(got) == len(want) == 26
    for j, (a, b) in enumerate(zip(got, want)):
        assert bytes(a) == bytes(b), f"output {j} differs from the manual route"
    plain = str(tmp_path / "plain.y4m")
    nsc.convert_y4m(src, plain, fps_out=60, window_frames=V.N, matrix="bt601")
    assert open(plain, "rb").read() != outs[3], "the flag does something"
    with pytest.raises(ValueError, match="flow_bidirectional needs method optical_flow"):
        nsc.convert_y4m(src, str(tmp_path / "c.y4m"), fps_out=60, method="blend", flow_bidirectional=True)
    assert not os.path.exists(tmp_path / "c.y4m")
