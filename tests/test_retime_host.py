"""The rate-conversion schedule without a GPU: nus_retime_count and nus_retime_schedule equal the restatement of tests/_retime.py,
the schedule's stated properties hold, windows tile the table, the Python mirror agrees, and every argument error of the retime
entry points is NUS_ERR_INVALID_ARGUMENT before any HIP call with a text that names the entry point."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import _retime

N_FRAMES = [2, 3, 7, 9]
RATIOS = [(5, 2), (12, 5), (2, 5), (1, 1), (8, 1), (1001, 400), (7, 3), (24, 5), (1, 3), (60, 24)]


def _table(lib, n_frames, num, den, first=0, count=None):
    n_out = lib.nus_retime_count(n_frames, num, den)
    assert n_out >= 0
    cnt = n_out - first if count is None else count
    buf = np.full((max(cnt, 1) + 1, 4), 0xA5A5A5A5, np.uint32)  # one row more: it must stay as it is
    assert lib.nus_retime_schedule(n_frames, num, den, first, cnt, buf.ctypes.data) == 0
    assert (buf[cnt:] == 0xA5A5A5A5).all()
    return buf[:cnt]


@pytest.mark.parametrize("num,den", RATIOS)
@pytest.mark.parametrize("n_frames", N_FRAMES)
def test_count_and_schedule_equal_the_restatement(nsc, n_frames, num, den):
    lib = nsc._capi.lib()
    want = _retime.schedule(n_frames, num, den)
    assert lib.nus_retime_count(n_frames, num, den) == _retime.count(n_frames, num, den) == len(want)
    got = _table(lib, n_frames, num, den)
    assert np.array_equal(got, _retime.as_array(want))
    rn, rd = _retime.reduce(num, den)
    ks = [k for k, _, _ in want]
    assert ks == sorted(ks) and ks[0] == 0 and want[0][1] == 0  # k_j is monotone; output 0 is frame 0
    per_pair = max(ks.count(k) for k in set(ks))
    assert per_pair <= -(-rn // rd)  # ceil(num / den)
    last_is_real = want[-1][0] == n_frames - 1
    assert last_is_real == (((n_frames - 1) * rn) % rd == 0)
    assert all(k <= n_frames - 2 or r == 0 for k, r, _ in want)  # only a real frame may name the last frame
    assert all(0.0 <= float(t) < 1.0 for _, _, t in want)


@pytest.mark.parametrize("num,den", RATIOS + [(4096, 4095), (4095, 4096), (4093, 512)])
def test_vectorised_restatement_equals_the_list(num, den):
    """_retime.schedule_array (numpy uint64, what the million-frame GPU test takes its reference from) against the list in Python
    ints, whole and in windows; and against Python ints again where j den is past 2^32."""
    for n in N_FRAMES + [700]:
        want = _retime.as_array(_retime.schedule(n, num, den))
        assert np.array_equal(_retime.schedule_array(n, num, den), want), (n, num, den)
        for first in (0, 1, len(want) // 2, len(want)):
            cnt = min(3, len(want) - first)
            assert np.array_equal(_retime.schedule_array(n, num, den, first, cnt), want[first:first + cnt]), (n, num, den, first)
    n = 1050000
    rn, rd = _retime.reduce(num, den)
    n_out = _retime.count(n, num, den)
    tail = _retime.schedule_array(n, num, den, n_out - 5, 5)
    for i, j in enumerate(range(n_out - 5, n_out)):
        k, r = (j * rd) // rn, (j * rd) % rn
        assert tail[i].tolist() == [k, r, int(np.float32(np.float64(r) / rn).view(np.uint32)), 0], (num, den, j)
    assert _retime.first_output(65535, num, den) == -(-65535 * rn // rd)
    assert np.array_equal(_retime.times_of(tail).view(np.uint32), tail[:, 2])


def test_host_table_at_the_bounds(nsc):
    """nus_retime_schedule where j * den passes 2^32 (a million frames at den 4095 and 4096): windows at the start, across
    j = 2^32 / den and at the end against the vectorised restatement."""
    lib = nsc._capi.lib()
    n = 1050000
    for num, den in [(4096, 4095), (4095, 4096)]:
        n_out = lib.nus_retime_count(n, num, den)
        assert n_out == _retime.count(n, num, den)
        across = (1 << 32) // den
        assert 32 <= across <= n_out - 64
        for first in (0, across - 32, n_out - 64):
            assert np.array_equal(_table(lib, n, num, den, first, 64), _retime.schedule_array(n, num, den, first, 64)), (num, den, first)


def test_block_matching_refuses_a_stream_that_would_need_a_second_launch(nsc):
    """nus_bm_retime_device_stream takes at most 65 535 pairs (its search has the pairs on one grid axis): 65 537 frames are refused
    before any HIP call, so the launch split of launch_retime_warp is never reached with block vectors."""
    lib = nsc._capi.lib()
    st, msg = _bm(nsc, lib, n_frames=65537)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT and msg.startswith("nus_bm_retime_device_stream:") and "too many" in msg, (st, msg)
    st, msg = _bm(nsc, lib, n_frames=65536, frames=None)  # 65 535 pairs pass that check (and fail the next one)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT and "too many" not in msg, (st, msg)


def test_reduced_ratio_gives_the_same_table(nsc):
    lib = nsc._capi.lib()
    for n in N_FRAMES:
        assert np.array_equal(_table(lib, n, 60, 24), _table(lib, n, 5, 2))
        assert np.array_equal(_table(lib, n, 4096, 4096), _table(lib, n, 1, 1))


@pytest.mark.parametrize("m", range(2, 9))
def test_integer_ratio_gives_frame_times_bit_for_bit(nsc, m):
    got = _table(nsc._capi.lib(), 4, m, 1)
    times = np.array(nsc.frame_times(m), np.float32).view(np.uint32)
    for k in range(3):
        rows = got[got[:, 0] == k]
        assert rows[0, 1] == 0 and np.array_equal(rows[1:, 2], times), (m, k)
    assert got[-1, 0] == 3 and got[-1, 1] == 0 and len(got) == 3 * m + 1


def test_every_time_is_the_float64_quotient_rounded_once(nsc):
    # every remainder of every num <= 1024 through nus_retime_schedule: with den coprime to num the remainders (j den) % num of
    # j = 0 .. num - 1 are all of 0 .. num - 1, and den + 1 frames give at least num outputs.  r / num in float64 and then to
    # float32 is the correctly rounded quotient (53 >= 2 * 24 + 2 bits: no double rounding), so it is what one f32 division gives.
    from math import gcd

    lib = nsc._capi.lib()
    for num in range(1, 1025):
        den = -(-num // 8)
        while gcd(num, den) != 1:
            den += 1
        got = _table(lib, den + 1, num, den)[:num]
        assert sorted(got[:, 1].tolist()) == list(range(num)), (num, den)
        want = (got[:, 1].astype(np.float64) / num).astype(np.float32).view(np.uint32)
        assert np.array_equal(got[:, 2], want), (num, den)


@pytest.mark.parametrize("num,den", [(5, 2), (1001, 400), (2, 5)])
def test_windows_tile_the_table(nsc, num, den):
    lib = nsc._capi.lib()
    n_frames = 9
    full = _table(lib, n_frames, num, den)
    for step in (1, 3, len(full)):
        parts = [_table(lib, n_frames, num, den, f, min(step, len(full) - f)) for f in range(0, len(full), step)]
        assert np.array_equal(np.concatenate(parts), full)
    assert len(_table(lib, n_frames, num, den, len(full), 0)) == 0
    assert lib.nus_retime_schedule(n_frames, num, den, len(full), 1, full.ctypes.data) == nsc._capi.ERR_INVALID_ARGUMENT
    assert nsc._capi.last_error().startswith("nus_retime_schedule:")


def test_python_mirror_equals_the_library(nsc):
    from nu_scaler_amd.retime import library_schedule, retime_count, retime_ratio, retime_schedule

    for fi, fo in [(24, 60), (25, 60), (30, 144), (60, 24), (Fraction(24000, 1001), 60), (400, 1001)]:
        num, den = retime_ratio(fi, fo)
        for n in N_FRAMES:
            mine = retime_schedule(n, fi, fo)
            assert len(mine) == retime_count(n, fi, fo)
            assert mine == library_schedule(n, num, den)
    for bad in [(0, 60), (24, 0), (24, 24 * 9), (1, Fraction(1, 4097)), (True, 2), (24.0, 60)]:
        with pytest.raises(ValueError):
            retime_ratio(*bad)
    with pytest.raises(ValueError):
        retime_count(1, 24, 60)


# ---- argument errors: every entry point, before any HIP call ---------------------------------------------------------------

BAD_RATIOS = [((0, 1), "non-zero"), ((1, 0), "non-zero"), ((4097, 4096), "at most 4096"), ((1, 4097), "at most 4096"), ((9, 1), "at most 8"),
              ((4096, 511), "at most 8")]
W, H = 6, 4
FB = W * H * 4
PTR = 0x10000  # never dereferenced: every call below fails its checks


def _interp(nsc, lib, n_frames=3, num=5, den=2, frames=PTR, stride=FB, out=PTR, out_stride=0, flows=None, w=W, h=H):
    it = nsc.WgpuFrameInterpolator()
    st = lib.nus_interp_retime_device(it._h, frames, stride, n_frames, flows, w, h, num, den, out, out_stride, None)
    return st, it._err()


def _flow(nsc, lib, n_frames=3, num=5, den=2, frames=PTR, out=PTR, out_stride=0, flows=None, fmt=0):
    fe = nsc.FlowEstimator()
    st = lib.nus_flow_retime_device_stream(fe._h, frames, n_frames, W, H, 1, 4, 2, ctypes.c_float(0.0004), num, den, fmt, flows, out,
                                           out_stride, None)
    return st, (lib.nus_flow_last_error(fe._h).decode() if fmt in (0, 1) else nsc._capi.last_error())


def _bm(nsc, lib, n_frames=3, num=5, den=2, frames=PTR, stride=FB, out=PTR, out_stride=0, ws=PTR, ws_bytes=1 << 30, mode=0):
    bm = nsc.BlockMatcher()
    st = lib.nus_bm_retime_device_stream(bm._h, frames, stride, n_frames, W, H, num, den, mode, ws, ws_bytes, None, out, out_stride, None)
    return st, lib.nus_bm_last_error(bm._h).decode()


def _scene(nsc, lib, n_frames=3, num=5, den=2, frames=PTR, stride=FB, out=PTR, out_stride=0, cut=PTR, fmt=0):
    st = lib.nus_scene_apply_cuts_retime_device(frames, stride, n_frames, W, H, fmt, num, den, cut, out, out_stride, None)
    return st, nsc._capi.last_error()


def _table_dev(nsc, lib, n_frames=3, num=5, den=2, out=PTR, **_):
    return lib.nus_retime_schedule_device(n_frames, num, den, out, None), nsc._capi.last_error()


ENTRY = {"nus_interp_retime_device": _interp, "nus_flow_retime_device_stream": _flow, "nus_bm_retime_device_stream": _bm,
         "nus_scene_apply_cuts_retime_device": _scene, "nus_retime_schedule_device": _table_dev}


@pytest.mark.parametrize("who", sorted(ENTRY))
def test_ratio_and_length_errors_are_refused_with_their_text(nsc, who):
    lib = nsc._capi.lib()
    for (num, den), text in BAD_RATIOS:
        st, msg = ENTRY[who](nsc, lib, num=num, den=den)
        assert st == nsc._capi.ERR_INVALID_ARGUMENT and msg.startswith(who + ":") and text in msg, (who, num, den, msg)
    for n in (0, 1):
        st, msg = ENTRY[who](nsc, lib, n_frames=n)
        assert st == nsc._capi.ERR_INVALID_ARGUMENT and msg.startswith(who + ":") and "at least 2 frames" in msg, (who, n, msg)


def test_host_entry_points_refuse_the_same_errors(nsc):
    lib = nsc._capi.lib()
    buf = np.zeros((64, 4), np.uint32)
    for (num, den), text in BAD_RATIOS:
        assert lib.nus_retime_count(3, num, den) == nsc._capi.ERR_INVALID_ARGUMENT
        msg = nsc._capi.last_error()
        assert msg.startswith("nus_retime_count:") and text in msg, msg
        assert lib.nus_retime_schedule(3, num, den, 0, 1, buf.ctypes.data) == nsc._capi.ERR_INVALID_ARGUMENT
        msg = nsc._capi.last_error()
        assert msg.startswith("nus_retime_schedule:") and text in msg, msg
    for n in (0, 1):
        assert lib.nus_retime_count(n, 5, 2) == nsc._capi.ERR_INVALID_ARGUMENT and "at least 2 frames" in nsc._capi.last_error()
    assert lib.nus_retime_schedule(3, 5, 2, 0, 1, None) == nsc._capi.ERR_INVALID_ARGUMENT
    assert (buf == 0).all()


@pytest.mark.parametrize("who", ["nus_interp_retime_device", "nus_bm_retime_device_stream", "nus_scene_apply_cuts_retime_device",
                                 "nus_flow_retime_device_stream"])
def test_stride_and_alignment_errors_are_refused(nsc, who):
    lib = nsc._capi.lib()
    call = ENTRY[who]
    bad = [dict(out_stride=FB - 4), dict(out_stride=FB + 2), dict(out=PTR + 2), dict(frames=PTR + 1), dict(frames=None), dict(out=None)]
    if who != "nus_flow_retime_device_stream":  # (its frames are tightly packed: no stride argument)
        bad += [dict(stride=FB - 4), dict(stride=FB + 2)]
    else:
        bad += [dict(out=PTR + 8), dict(flows=PTR + 8), dict(fmt=2)]
    if who == "nus_interp_retime_device":
        bad += [dict(flows=PTR + 4), dict(w=0)]
    if who == "nus_bm_retime_device_stream":
        bad += [dict(ws=PTR + 8), dict(ws_bytes=16), dict(mode=2), dict(ws=None)]
    if who == "nus_scene_apply_cuts_retime_device":
        bad += [dict(cut=None), dict(fmt=4)]
    for kw in bad:
        st, msg = call(nsc, lib, **kw)
        assert st == nsc._capi.ERR_INVALID_ARGUMENT and msg.startswith(who + ":"), (who, kw, st, msg)


def test_python_wrappers_raise_before_any_gpu_work(nsc):
    with pytest.raises(ValueError, match="nus_interp_retime_device"):
        nsc.WgpuFrameInterpolator().retime_device(PTR, FB, 3, 0, W, H, 9, 1, PTR)
    with pytest.raises((ValueError, RuntimeError), match="nus_flow_retime_device_stream"):
        nsc.FlowEstimator().retime_device_stream(PTR, 3, W, H, 9, 1, PTR)
    with pytest.raises((ValueError, RuntimeError), match="nus_bm_retime_device_stream"):
        nsc.BlockMatcher().retime_stream_device(PTR, FB, 3, W, H, 9, 1, PTR, 1 << 30, PTR)


# ---- `retime` of both command-line tools: usage errors give status 2 before anything is read or written --------------------

BAD_COMMANDS = [
    ["--from", "24", "--to", "60", "OUT_%04d.png", "missing0.png"],                        # one input frame
    ["--from", "24", "--to", "60", "OUT.png", "missing0.png", "missing1.png"],             # no %d in the pattern
    ["--from", "24", "--to", "60", "OUT_%d_%d.png", "missing0.png", "missing1.png"],       # two conversions
    ["--from", "24", "--to", "0", "OUT_%04d.png", "missing0.png", "missing1.png"],         # a zero rate
    ["--from", "1", "--to", "9", "OUT_%04d.png", "missing0.png", "missing1.png"],          # a ratio above 8
    ["--from", "4097", "--to", "4096", "OUT_%04d.png", "missing0.png", "missing1.png"],    # a term above the bound
    ["--from", "x", "--to", "60", "OUT_%04d.png", "missing0.png", "missing1.png"],
    ["--to", "60", "OUT_%04d.png", "missing0.png", "missing1.png"],                        # no --from
    ["--from", "24", "--to", "60", "--method", "median", "OUT_%04d.png", "missing0.png", "missing1.png"],
    ["--from", "24", "--to", "60", "--method", "blend", "--flow-warps", "1", "OUT_%04d.png", "missing0.png", "missing1.png"],
    ["--from", "24", "--to", "60", "--flow-median", "4", "OUT_%04d.png", "missing0.png", "missing1.png"],
    ["--from", "24", "--to", "60", "--flow-project", "5", "OUT_%04d.png", "missing0.png", "missing1.png"],
    ["--from", "24", "--to", "60", "--bidirectional", "OUT_%04d.png", "missing0.png", "missing1.png"],
]


@pytest.mark.parametrize("tool", ["python", "native"])
def test_cli_usage_errors_give_status_2_and_touch_no_file(nsc, tmp_path, tool):
    import os
    import subprocess
    import sys

    from conftest import ROOT

    argv = [sys.executable, "-m", "nu_scaler_amd.cli"] if tool == "python" else [os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for bad in BAD_COMMANDS:
        # (the inputs do not exist: a command that got as far as reading them would end with status 1)
        r = subprocess.run(argv + ["retime"] + bad, capture_output=True, text=True, cwd=tmp_path, env=env, timeout=120)
        assert r.returncode == 2, (tool, bad, r.returncode, r.stderr[-300:])
        assert os.listdir(tmp_path) == [], (tool, bad)
    r = subprocess.run(argv + ["retime", "--from", "24", "--to", "60", "OUT_%04d.png", "missing0.png", "missing1.png"], capture_output=True,
                       text=True, cwd=tmp_path, env=env, timeout=120)
    assert r.returncode == 1 and os.listdir(tmp_path) == [], (tool, r.returncode, r.stderr[-300:])  # a good command fails at the read
