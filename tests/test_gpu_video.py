"""`convert_y4m` and the `video` sub-command on the MI355X: a synthetic 64 x 48 clip (a square moving over a gradient, 11 frames
at 24 fps) converted window by window gives the same file for every window size, every frame of it equals the manual route --
`yuv.to_rgba` per frame, `retime.retime_frames` over the whole clip with handles of the same settings, `yuv.to_yuv` per frame --
and the header carries the new rate and the input's other tags; the same at 60 -> 24 (den = 5) for the blend and the block
matcher; `multiplier=2, scale=2` against the upscaler applied to the unscaled run's RGBA; the CLI as a child process."""
import functools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import _yuv as Y
from conftest import ROOT
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 11


@functools.lru_cache(maxsize=None)
def _clip(matrix=Y.BT601, rng=Y.FULL, siting=Y.LEFT):
    """N I420 frames: a bright square that moves 3 px right and 1 px down a frame over a static colour gradient."""
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    frames = []
    for k in range(N):
        rgb = np.stack([40 + 3 * x, 30 + 4 * y, 200 - 2 * x - y], axis=-1).astype(np.uint8)
        x0, y0 = 4 + 3 * k, 6 + k
        rgb[y0:y0 + 14, x0:x0 + 14] = (250, 240, 60)
        frames.append(Y.to_yuv(rgb, matrix, rng, siting).tobytes())
    return tuple(frames)


def _write_clip(path, header, frames):
    with open(path, "wb") as fh:
        fh.write(header + b"\n")
        for f in frames:
            fh.write(b"FRAME\n" + f)
    return str(path)


def _read(path):
    from nu_scaler_amd.y4m import Y4MReader

    data = open(path, "rb").read()
    with Y4MReader(path) as r:
        return data[:data.index(b"\n")], list(r)


def _manual(nsc, frames, fmt, fps_in, fps_out, method, **kw):
    """The route without windows: host conversions around retime_frames over the whole clip."""
    from nu_scaler_amd.retime import retime_frames

    rgba = [nsc.yuv.to_rgba(f, W, H, fmt) for f in frames]
    if method == "block_matching":
        out = retime_frames(rgba, W, H, fps_in, fps_out, matcher=nsc.BlockMatcher("medium", bidirectional=kw.get("bidirectional", False)))
    else:
        flow = nsc.FlowEstimator() if method == "optical_flow" else None
        out = retime_frames(rgba, W, H, fps_in, fps_out, warp=nsc.WgpuFrameInterpolator(), flow=flow)
    return out, [nsc.yuv.to_yuv(o, W, H, fmt) for o in out]


def test_24_to_60_is_the_same_file_for_every_window_and_equals_the_manual_route(nsc, tmp_path):
    frames = _clip()
    src = _write_clip(tmp_path / "in.y4m", b"YUV4MPEG2 W64 H48 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL", frames)
    outs = {}
    for win in (3, 5, N):
        out = str(tmp_path / f"out{win}.y4m")
        r = nsc.convert_y4m(src, out, fps_out=60, window_frames=win, matrix="bt601")
        assert (r["frames_in"], r["frames_out"], r["fps"], r["width"], r["height"]) == (N, 26, Fraction(60), W, H)
        assert r["windows"] == len(nsc.plan_windows(N, 5, 2, win)) == {3: 5, 5: 3, N: 1}[win]
        outs[win] = open(out, "rb").read()
    assert outs[3] == outs[5] == outs[N]
    header, got = _read(str(tmp_path / "out3.y4m"))
    assert header == b"YUV4MPEG2 W64 H48 F60:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL"
    fmt = nsc.YuvFormat("bt601", "full", "left", "bilinear")
    _, want = _manual(nsc, frames, fmt, 24, 60, "optical_flow")
    assert len(got) == len(want) == 26
    for j, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"output {j} differs from the manual route"
    assert got[0] != got[1] and got[5] != got[10]  # (the clip moves)
    # the default window comes from the device's free memory and holds this clip whole
    out = str(tmp_path / "auto.y4m")
    assert nsc.convert_y4m(src, out, fps_out=60, matrix="bt601")["windows"] == 1
    assert open(out, "rb").read() == outs[3]


@pytest.mark.parametrize("method", ("blend", "block_matching"))
def test_60_to_24_in_windows_of_six(nsc, tmp_path, method):
    """den = 5: a window holds 6 frames, the clip two windows; untagged input: centre siting, limited range, BT.601 by its height."""
    frames = _clip(Y.BT601, Y.LIMITED, Y.CENTER)
    src = _write_clip(tmp_path / "in.y4m", b"YUV4MPEG2 W64 H48 F60:1", frames)
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    ra = nsc.convert_y4m(src, a, fps_out=24, window_frames=6, method=method)
    rb = nsc.convert_y4m(src, b, fps_out=24, window_frames=N, method=method)
    assert (ra["windows"], rb["windows"], ra["frames_out"], rb["frames_out"]) == (2, 1, 5, 5)
    assert open(a, "rb").read() == open(b, "rb").read()
    header, got = _read(a)
    assert header == b"YUV4MPEG2 W64 H48 F24:1"
    _, want = _manual(nsc, frames, nsc.YuvFormat("bt601", "limited", "center", "bilinear"), 60, 24, method)
    assert got == want
    with pytest.raises(ValueError, match="den \\+ 1 = 6"):
        nsc.convert_y4m(src, str(tmp_path / "c.y4m"), fps_out=24, window_frames=5, method=method)
    if method == "blend":
        with pytest.raises(ValueError, match="bidirectional needs method block_matching"):
            nsc.convert_y4m(src, str(tmp_path / "c.y4m"), fps_out=24, method=method, bidirectional=True)


def test_multiplier_two_scale_two_equals_the_upscaler_on_the_unscaled_rgba(nsc, tmp_path):
    import torch

    frames = _clip(Y.BT601, Y.LIMITED, Y.CENTER)[:5]
    src = _write_clip(tmp_path / "in.y4m", b"YUV4MPEG2 W64 H48 F30000:1001 C420jpeg", frames)
    out = str(tmp_path / "big.y4m")
    r = nsc.convert_y4m(src, out, multiplier=2, scale=2, method="blend", window_frames=3)
    assert (r["frames_out"], r["width"], r["height"], r["fps"], r["windows"]) == (9, 2 * W, 2 * H, Fraction(60000, 1001), 2)
    header, got = _read(out)
    assert header == b"YUV4MPEG2 W128 H96 F60000:1001 C420jpeg"
    fmt = nsc.YuvFormat("bt601", "limited", "center", "bilinear")
    rgba, _ = _manual(nsc, frames, fmt, 1, 2, "blend")
    up = nsc.PyWgpuUpscaler("quality", "lanczos3")
    up.initialize(W, H, 2 * W, 2 * H)
    d_in = put(np.stack([np.frombuffer(f, np.uint8) for f in rgba]), "cuda:0")
    d_out = torch.empty((len(rgba), 4 * W * H * 4), dtype=torch.uint8, device="cuda:0")
    up.upscale_device(d_in.data_ptr(), d_out.data_ptr(), len(rgba), torch.cuda.current_stream().cuda_stream)
    big = fetch(d_out)
    want = [nsc.yuv.to_yuv(big[j].tobytes(), 2 * W, 2 * H, fmt) for j in range(len(rgba))]
    assert len(got) == 9 and got == want


def test_video_sub_command_as_a_child_process(nsc, tmp_path):
    frames = _clip()
    src = _write_clip(tmp_path / "in.y4m", b"YUV4MPEG2 W64 H48 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL", frames)
    want, got = str(tmp_path / "want.y4m"), str(tmp_path / "got.y4m")
    nsc.convert_y4m(src, want, fps_out=Fraction(60), window_frames=5, method="blend", matrix="bt709")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "nu_scaler_amd.cli", "video", src, got, "--to", "60/1", "--window", "5", "--method", "blend",
                        "--matrix", "bt709"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "26 frames 64x48 at 60 fps (11 read, 3 windows)" in r.stdout
    assert open(got, "rb").read() == open(want, "rb").read()
