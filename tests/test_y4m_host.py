"""Y4M files and the window plan without a GPU (nu_scaler_amd/y4m.py, video.plan_windows, the `video` sub-command's usage
errors): every accepted header tag and every refused one with the text that names it, 30000:1001 kept exactly, FRAME lines with
parameters, truncated frames, a byte-identical writer -> reader round trip; the windows tile the input, start at multiples of
den and their kept outputs are, entry for entry, the schedule of the whole stream (tests/_retime.py)."""
import os
import subprocess
import sys
from fractions import Fraction

import pytest

import _retime
from conftest import ROOT
from nu_scaler_amd import y4m
from nu_scaler_amd.video import check_convert_args, default_matrix, plan_windows, window_bytes_per_frame


def _file(tmp_path, header, frames=(), name="a.y4m", frame_line=b"FRAME\n"):
    p = tmp_path / name
    p.write_bytes(header + b"\n" + b"".join(frame_line + f for f in frames))
    return str(p)


def test_header_tags_that_are_accepted(tmp_path):
    f = bytes(range(6))  # 2 x 2: 4 + 1 + 1 bytes
    cases = [(b"YUV4MPEG2 W2 H2 F24:1", "center", "limited", None, None, None),
             (b"YUV4MPEG2 W2 H2 F24:1 C420", "center", "limited", None, None, "420"),
             (b"YUV4MPEG2 W2 H2 F25:1 Ip A1:1 C420jpeg", "center", "limited", "p", "1:1", "420jpeg"),
             (b"YUV4MPEG2 W2 H2 F30000:1001 I? A0:0 C420mpeg2 XYSCSS=420MPEG2", "left", "limited", "?", "0:0", "420mpeg2"),
             (b"YUV4MPEG2 W2 H2 F60:1 Ip C420jpeg XCOLORRANGE=FULL", "center", "full", "p", None, "420jpeg"),
             (b"YUV4MPEG2 H2 W2 F60:1 XCOLORRANGE=LIMITED XFOO=1", "center", "limited", None, None, None)]
    for hdr, siting, rng, il, aspect, cs in cases:
        with y4m.Y4MReader(_file(tmp_path, hdr, [f, f])) as r:
            assert (r.width, r.height, r.siting, r.range, r.interlace, r.aspect, r.colorspace) == (2, 2, siting, rng, il, aspect, cs), hdr
            assert r.tags == hdr.decode().split(" ")[1:] and r.frame_bytes == 6
            assert list(r) == [f, f] and r.frames_read == 2
    with y4m.Y4MReader(_file(tmp_path, cases[3][0])) as r:
        assert r.fps == Fraction(30000, 1001) and (r.fps.numerator, r.fps.denominator) == (30000, 1001)
        assert r.x_tags == ["YSCSS=420MPEG2"] and r.read_frame() is None


@pytest.mark.parametrize("tag,text", [("C420paldv", "C420paldv"), ("C422", "C422"), ("C444", "C444"), ("Cmono", "Cmono"), ("C420p10", "C420p10"),
                                      ("C422p12", "C422p12"), ("C444p16", "C444p16"), ("C420p12", "C420p12"), ("It", "It"), ("Ib", "Ib"),
                                      ("Im", "Im"), ("XCOLORRANGE=VIDEO", "XCOLORRANGE=VIDEO"), ("A1-1", "A1-1"), ("F24", "F24"), ("F24:0", "F24:0"),
                                      ("W0", "W0"), ("Hx", "Hx")])
def test_header_tags_that_are_refused_name_the_tag(tmp_path, tag, text):
    base = ["W2", "H2", "F24:1"]
    words = [w for w in base if w[0] != tag[0]] + [tag]
    with pytest.raises(ValueError, match="Y4M tag " + text.replace("?", r"\?")):
        y4m.Y4MReader(_file(tmp_path, ("YUV4MPEG2 " + " ".join(words)).encode()))


def test_missing_tags_and_bad_files(tmp_path):
    for missing in "WHF":
        words = [w for w in ("W2", "H2", "F24:1") if w[0] != missing]
        with pytest.raises(ValueError, match=f"the {missing} tag is missing"):
            y4m.Y4MReader(_file(tmp_path, ("YUV4MPEG2 " + " ".join(words)).encode()))
    with pytest.raises(ValueError, match="does not begin with YUV4MPEG2"):
        y4m.Y4MReader(_file(tmp_path, b"YUV4MPEG W2 H2 F1:1"))
    p = tmp_path / "empty.y4m"
    p.write_bytes(b"")
    with pytest.raises(ValueError, match="empty"):
        y4m.Y4MReader(str(p))
    with pytest.raises(OSError):
        y4m.Y4MReader(str(tmp_path / "absent.y4m"))


def test_frame_lines_with_parameters_and_truncated_frames(tmp_path):
    f0, f1 = bytes(range(27)), bytes(range(100, 127))  # 5 x 3
    hdr = b"YUV4MPEG2 W5 H3 F24:1 C420jpeg"
    with y4m.Y4MReader(_file(tmp_path, hdr, [f0, f1], frame_line=b"FRAME Ip XQ=1\n")) as r:
        assert r.read_frames(5) == [f0, f1]
    with y4m.Y4MReader(_file(tmp_path, hdr, [f0, f1[:-1]])) as r:
        assert r.read_frame() == f0
        with pytest.raises(ValueError, match="frame 1 is truncated: 26 of 27 bytes"):
            r.read_frame()
    with y4m.Y4MReader(_file(tmp_path, hdr, [f0], frame_line=b"FRAMES\n")) as r:
        with pytest.raises(ValueError, match="expected a FRAME line"):
            r.read_frame()
    p = tmp_path / "cut.y4m"
    p.write_bytes(hdr + b"\nFRAME\n" + f0 + b"FRA")
    with y4m.Y4MReader(str(p)) as r:
        assert r.read_frame() == f0
        with pytest.raises(ValueError, match="without its newline"):
            r.read_frame()


def test_writer_reader_round_trip_is_byte_identical(tmp_path):
    frames = [bytes((7 * k + i) % 256 for i in range(27)) for k in range(3)]
    src = _file(tmp_path, b"YUV4MPEG2 W5 H3 F30000:1001 Ip A128:117 C420mpeg2 XCOLORRANGE=FULL", frames)
    with y4m.Y4MReader(src) as r:
        out = str(tmp_path / "b.y4m")
        with y4m.Y4MWriter(out, r.width, r.height, r.fps, r.siting, r.range, r.aspect, r.interlace, r.colorspace) as w:
            for f in r:
                w.write(f)
            assert w.frames_written == 3
    assert open(out, "rb").read() == open(src, "rb").read()
    # the defaults: the tag of the siting, nothing optional
    out = str(tmp_path / "c.y4m")
    with y4m.Y4MWriter(out, 5, 3, 24) as w:
        w.write(frames[0])
        with pytest.raises(ValueError, match="holds 27 bytes, got 26"):
            w.write(frames[0][:-1])
    assert open(out, "rb").read() == b"YUV4MPEG2 W5 H3 F24:1 C420jpeg\nFRAME\n" + frames[0]
    with y4m.Y4MWriter(out, 5, 3, Fraction(60000, 1001), "left", "limited", "1:1") as w:
        pass
    assert open(out, "rb").read() == b"YUV4MPEG2 W5 H3 F60000:1001 A1:1 C420mpeg2 XCOLORRANGE=LIMITED\n"
    for kw, text in ((dict(siting="top"), "siting"), (dict(range="tv"), "range"), (dict(interlace="t"), "interlace"),
                     (dict(colorspace="420mpeg2"), "colorspace"), (dict(siting="left", colorspace=None), "colorspace")):
        with pytest.raises(ValueError, match=text):
            y4m.Y4MWriter(str(tmp_path / "never.y4m"), 5, 3, 24, **kw)
    with pytest.raises(ValueError, match="positive"):
        y4m.Y4MWriter(str(tmp_path / "never.y4m"), 0, 3, 24)
    assert not os.path.exists(str(tmp_path / "never.y4m"))


RATIOS = [(5, 2), (2, 5), (12, 5), (2, 1), (1, 1), (24, 5)]


@pytest.mark.parametrize("num,den", RATIOS)
def test_plan_windows_tiles_the_stream_and_keeps_its_schedule(num, den):
    for n in range(2, 24):
        whole = _retime.schedule(n, num, den)
        assert len(whole) == _retime.count(n, num, den)
        for max_frames in (den + 1, den + 2, 2 * den + 1, 7, 11, 23, 64):
            if max_frames < den + 1:
                continue
            plan = plan_windows(n, num, den, max_frames)
            assert plan == plan_windows(n, 3 * num, 3 * den, max_frames)  # the ratio is reduced
            got, end = [], 0
            for i, (first, count, first_out, kept) in enumerate(plan):
                last = i == len(plan) - 1
                assert first % den == 0 and 2 <= count <= max_frames and first == end and first_out == len(got)
                assert first_out * den == first * num  # the window's first output is its first frame
                if not last:
                    assert (count - 1) % den == 0 and count == (max_frames - 1) // den * den + 1
                local = _retime.schedule(count, num, den)
                assert kept == (len(local) if last else len(local) - 1)
                if not last:
                    assert local[-1][0] == count - 1 and local[-1][1] == 0  # the dropped output is the shared real frame
                got += [(first + k, r, t) for k, r, t in local[:kept]]
                end = first + count - 1
            assert end == n - 1
            assert len(got) == len(whole)
            assert [(k, r) for k, r, _ in got] == [(k, r) for k, r, _ in whole]
            assert all(a[2] == b[2] for a, b in zip(got, whole))  # the same float32 times
    assert plan_windows(11, 5, 2, 3) == [(0, 3, 0, 5), (2, 3, 5, 5), (4, 3, 10, 5), (6, 3, 15, 5), (8, 3, 20, 6)]
    assert plan_windows(11, 5, 2, 5) == [(0, 5, 0, 10), (4, 5, 10, 10), (8, 3, 20, 6)]
    assert plan_windows(11, 5, 2, 11) == plan_windows(11, 5, 2, 400) == [(0, 11, 0, 26)]
    assert plan_windows(11, 2, 5, 6) == [(0, 6, 0, 2), (5, 6, 2, 3)]


def test_plan_windows_refuses():
    for args, text in (((1, 5, 2, 9), "at least 2 frames"), ((9, 5, 2, 2), "den \\+ 1 = 3"), ((9, 2, 5, 5), "den \\+ 1 = 6"),
                       ((9, 0, 2, 9), "positive terms"), ((9, 10, 4, 2), "den \\+ 1 = 3")):
        with pytest.raises(ValueError, match=text):
            plan_windows(*args)


def test_convert_arguments_and_defaults():
    assert check_convert_args(Fraction(24), 60, None, "optical_flow", 1, False) == (Fraction(60), 5, 2)
    assert check_convert_args(Fraction(30000, 1001), None, 2, "blend", 2, False) == (Fraction(60000, 1001), 2, 1)
    assert check_convert_args(Fraction(60), Fraction(24), None, "block_matching", 1, True) == (Fraction(24), 2, 5)
    for args, text in (((24, None, None, "blend", 1, False), "fps_out or multiplier"), ((24, 60, 2, "blend", 1, False), "fps_out or multiplier"),
                       ((24, None, 9, "blend", 1, False), "multiplier must be"), ((24, 60, None, "nearest", 1, False), "method must be"),
                       ((24, 60, None, "blend", 1, True), "bidirectional needs method block_matching"),
                       ((24, 60, None, "optical_flow", 1, True), "bidirectional needs method block_matching"),
                       ((24, 60, None, "blend", 5, False), "scale must be"), ((24, 240, None, "blend", 1, False), "above 8"),
                       ((24, 0, None, "blend", 1, False), "positive")):
        with pytest.raises(ValueError, match=text):
            check_convert_args(Fraction(args[0]), *args[1:])
    assert default_matrix(1080) == default_matrix(720) == "bt709" and default_matrix(719) == default_matrix(48) == "bt601"
    # 1080p, 24 -> 60, no up-scale: 1.5 + 4 bytes a pixel in, 2.5 x (4 + 1.5) out
    assert window_bytes_per_frame(1920, 1080, 5, 2, 1) == 1920 * 1080 * (1.5 + 4 + 2.5 * 5.5)
    assert window_bytes_per_frame(64, 48, 1, 1, 2) == 64 * 48 * (1.5 + 4 + 4 + 16 + 6)


def _cli(*argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "nu_scaler_amd.cli", "video", *argv], capture_output=True, text=True, env=env, cwd=ROOT)


def test_video_usage_errors(tmp_path):
    """Status 2 and a one-line reason, before anything is read: the input below does not exist."""
    a, b = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    for argv, text in (([a, b], "video needs --to or --multiplier, one of them"), ([a, b, "--to", "60", "--multiplier", "2"], "one of them"),
                       ([a, b, "--to", "sixty"], "a rate is an integer or a fraction A/B"), ([a, b, "--to", "60/1/1"], "a rate is"),
                       ([a, b, "--multiplier", "9"], "--multiplier must be from 1 to 8, got 9"), ([a, b, "--to", "60", "--method", "warp"], "--method must be"),
                       ([a, b, "--to", "60", "--method", "blend", "--flow-warps", "1"], "--flow-warps needs --method optical_flow"),
                       ([a, b, "--to", "60", "--flow-median", "4"], "--flow-median: 4 is out of range"),
                       ([a, b, "--to", "60", "--flow-project", "5"], "--flow-project: 5 is out of range"),
                       ([a, b, "--to", "60", "--bidirectional"], "--bidirectional needs --method block_matching"),
                       ([a, b, "--to", "60", "--scale", "5"], "--scale must be from 1 to 4"), ([a, b, "--to", "60", "--matrix", "bt2020"], "--matrix must be"),
                       ([a, b, "--to", "60", "--window", "1"], "--window must be at least 2"), ([a], "the following arguments are required")):
        r = _cli(*argv)
        assert r.returncode == 2, (argv, r.stderr)
        assert "nu_scaler_cli" in r.stderr and ": error: " in r.stderr and text in r.stderr, (argv, r.stderr)
        assert not os.path.exists(b)
    r = _cli(a, b, "--to", "60")  # a usable command line: the missing file is a run-time error, status 1
    assert r.returncode == 1 and "nu_scaler_cli: error: " in r.stderr and "in.y4m" in r.stderr
    help_text = _cli("--help").stdout
    for opt in ("--to", "--multiplier", "--method", "--scale", "--algorithm", "--matrix", "--window", "--scene-detect", "--flow-warps",
                "--flow-median", "--flow-project", "--bidirectional", "--device"):
        assert opt in help_text, opt
