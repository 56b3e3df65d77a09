"""`convert_y4m(..., scale_domain="yuv")` and `video --scale-domain yuv` on the MI355X, over a synthetic 64 x 48 clip of 5 frames
(a square moving over a gradient): the planar route writes, frame for frame and byte for byte, `yuv.YuvResizer(.., siting=<the
clip's>).resize` of the frames the unscaled conversion writes, under the header the RGBA route writes, for a 420mpeg2 and a
420jpeg clip and for windows of 3 and of all frames; at the ratio 1/1 the up-scale of every input frame; "rgb" stays the default;
the CLI flag as a child process."""
import functools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import _yuv as Y
from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 5
CLIPS = {"left": (b"YUV4MPEG2 W64 H48 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL", Y.LEFT),
         "center": (b"YUV4MPEG2 W64 H48 F24:1 Ip A1:1 C420jpeg", Y.CENTER)}


@functools.lru_cache(maxsize=None)
def _clip(siting):
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    frames = []
    for k in range(N):
        rgb = np.stack([40 + 3 * x, 30 + 4 * y, 200 - 2 * x - y], axis=-1).astype(np.uint8)
        x0, y0 = 4 + 5 * k, 6 + 2 * k
        rgb[y0:y0 + 14, x0:x0 + 14] = (250, 240, 60)
        frames.append(Y.to_yuv(rgb, Y.BT601, Y.FULL, siting).tobytes())
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


@pytest.mark.parametrize("siting", ("left", "center"))
def test_the_planar_route_is_the_plane_resize_of_the_unscaled_conversion(nsc, tmp_path, siting):
    header, s = CLIPS[siting]
    src = _write_clip(tmp_path / "in.y4m", header, _clip(s))
    small, rgb = str(tmp_path / "small.y4m"), str(tmp_path / "rgb.y4m")
    nsc.convert_y4m(src, small, fps_out=60, method="blend", scale=1)
    nsc.convert_y4m(src, rgb, fps_out=60, method="blend", scale=2)
    rgb_header, rgb_frames = _read(rgb)
    _, base = _read(small)
    resizer = nsc.yuv.YuvResizer(W, H, 2 * W, 2 * H, siting=siting)
    want = [resizer.resize(f) for f in base]
    assert len(want) == 11
    files = {}
    for win in (3, N):
        out = str(tmp_path / f"yuv{win}.y4m")
        r = nsc.convert_y4m(src, out, fps_out=60, method="blend", scale=2, scale_domain="yuv", window_frames=win)
        assert (r["frames_in"], r["frames_out"], r["fps"], r["width"], r["height"]) == (N, 11, Fraction(60), 2 * W, 2 * H)
        assert r["windows"] == {3: 2, N: 1}[win]
        got_header, got = _read(out)
        assert got_header == rgb_header
        assert len(got) == len(want)
        for j, (a, b) in enumerate(zip(got, want)):
            assert a == b, f"{siting} window {win}: output {j} is not the plane resize of the unscaled output"
        files[win] = open(out, "rb").read()
    assert files[3] == files[N]
    assert len(rgb_frames) == 11 and rgb_frames != want  # (the two routes are different resamplings)
    # bicubic goes to the resizer too
    out = str(tmp_path / "cubic.y4m")
    nsc.convert_y4m(src, out, fps_out=60, method="blend", scale=2, algorithm="bicubic", scale_domain="yuv")
    cubic = nsc.yuv.YuvResizer(W, H, 2 * W, 2 * H, "bicubic", siting)
    assert _read(out)[1] == [cubic.resize(f) for f in base]


def test_ratio_one_is_the_plane_resize_of_every_input_frame(nsc, tmp_path):
    header, s = CLIPS["left"]
    frames = _clip(s)
    src = _write_clip(tmp_path / "in.y4m", header, frames)
    resizer = nsc.yuv.YuvResizer(W, H, 2 * W, 2 * H, siting="left")
    want = [resizer.resize(f) for f in frames]
    for win, method in ((2, "optical_flow"), (3, "block_matching"), (N, "blend")):  # `method` is not consulted
        out = str(tmp_path / f"one{win}.y4m")
        r = nsc.convert_y4m(src, out, multiplier=1, scale=2, scale_domain="yuv", window_frames=win, method=method)
        assert (r["frames_in"], r["frames_out"], r["fps"], r["width"], r["height"]) == (N, N, Fraction(24), 2 * W, 2 * H)
        got_header, got = _read(out)
        assert got_header == b"YUV4MPEG2 W128 H96 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL"
        assert got == want, f"window {win}"


def test_rgb_is_the_default(nsc, tmp_path):
    header, s = CLIPS["left"]
    src = _write_clip(tmp_path / "in.y4m", header, _clip(s))
    a, b, c = (str(tmp_path / n) for n in ("a.y4m", "b.y4m", "c.y4m"))
    nsc.convert_y4m(src, a, fps_out=60, method="blend", scale=2)
    nsc.convert_y4m(src, b, fps_out=60, method="blend", scale=2, scale_domain="rgb")
    assert open(a, "rb").read() == open(b, "rb").read()
    nsc.convert_y4m(src, a, fps_out=60, method="blend")  # without a scale the keyword changes nothing
    nsc.convert_y4m(src, c, fps_out=60, method="blend", scale_domain="yuv")
    assert open(a, "rb").read() == open(c, "rb").read()


def test_cli_scale_domain_yuv_as_a_child_process(nsc, tmp_path):
    header, s = CLIPS["left"]
    src = _write_clip(tmp_path / "in.y4m", header, _clip(s))
    want, got = str(tmp_path / "want.y4m"), str(tmp_path / "got.y4m")
    nsc.convert_y4m(src, want, fps_out=Fraction(60), window_frames=3, method="blend", scale=2, scale_domain="yuv")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "nu_scaler_amd.cli", "video", src, got, "--to", "60", "--window", "3", "--method", "blend",
                        "--scale", "2", "--scale-domain", "yuv"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "11 frames 128x96 at 60 fps (5 read, 2 windows)" in r.stdout
    assert open(got, "rb").read() == open(want, "rb").read()
