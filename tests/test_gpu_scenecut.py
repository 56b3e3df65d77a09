"""Scene-cut detector on the MI355X against the numpy yardstick (tests/_scenecut.py): measures, flags and the cut-aware output
rule are integer work, so everything is compared for equality -- no tolerance anywhere.  Device outputs live in
conftest.guarded tensors and come down through nus_download."""
import functools

import numpy as np
import pytest

import _scenecut as sc
from _scenecut_content import brighter, decision_cases, sine_pattern
from conftest import guarded
from nu_scaler_amd.interpolator import frame_times
from nu_scaler_amd.scene import MEASURES_DTYPE
from nu_scaler_amd.synthetic import gradient_frame, noise_frame
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

POISON = 0xA7  # conftest.guarded's fill of an `empty` tensor


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _frame(w, h, kind):
    """Frame number `kind` of a family with per-frame different content (and different alpha, which must not matter)."""
    m = kind % 6
    if m == 0:
        f = noise_frame(w, h, 0x5EED + kind)
    elif m == 1:
        f = gradient_frame(w, h, 3 * kind)
    elif m == 2:
        f = sine_pattern(w, h, float(kind))
    elif m == 3:
        f = brighter(sine_pattern(w, h, 0.0), 8 + kind)
    elif m == 4:
        f = np.full((h, w, 4), (7 * kind) % 256, np.uint8)
    else:
        f = sine_pattern(w, h, 2.0).copy()
        f[..., :3] //= 3
    f = np.ascontiguousarray(f).copy()
    f[..., 3] = (kind * 37) % 256
    return f


@functools.lru_cache(maxsize=None)
def _pairs(w, h, n):
    a = np.stack([_frame(w, h, 2 * i) for i in range(n)])
    b = np.stack([_frame(w, h, 2 * i + 1 + (i % 3)) for i in range(n)])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _detect(nsc, d_a, a_stride, d_b, b_stride, w, h, n, fmt="rgba", mad=20, hist=400, stream=None):
    """-> (measures (n,) MEASURES_DTYPE, cut (n,) uint8), from guarded tensors."""
    import torch

    det = nsc.SceneDetector(mad, hist)
    ws_bytes = det.workspace_size(w, h, n)
    ws = guarded.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    meas = guarded.empty(16 * n, dtype=torch.uint8, device="cuda:0")
    cut = guarded.empty(n, dtype=torch.uint8, device="cuda:0")
    det.detect_device(d_a, a_stride, d_b, b_stride, w, h, n, ws.data_ptr(), ws_bytes, cut.data_ptr(), meas.data_ptr(), fmt,
                      _stream() if stream is None else stream)
    return fetch(meas).view(MEASURES_DTYPE), fetch(cut)


def _want(a, b, fmt=sc.RGBA, mad=20, hist=400):
    h, w = a.shape[1:3]
    m = [sc.measures(x, y, fmt) for x, y in zip(a, b)]
    return m, [1 if sc.is_cut(s, l, w, h, mad, hist) else 0 for s, l in m]


def _assert_equal(meas, cut, want_m, want_c):
    assert [(int(s), int(l)) for s, l in zip(meas["sad"], meas["hist_l1"])] == want_m
    assert (meas["reserved"] == 0).all()
    assert cut.tolist() == want_c


@pytest.mark.parametrize("w,h", [(1, 1), (17, 9), (321, 183), (1920, 1080)])
@pytest.mark.parametrize("n", [1, 5, 32])
def test_measures_and_flags_equal_the_yardstick(nsc, w, h, n):
    a, b = _pairs(w, h, n)
    fb = w * h * 4
    da, db = put(a, "cuda:0"), put(b, "cuda:0")  # (named: a temporary's memory would be handed to the next tensor)
    meas, cut = _detect(nsc, da.data_ptr(), fb, db.data_ptr(), fb, w, h, n)
    _assert_equal(meas, cut, *_want(a, b))


@pytest.mark.parametrize("w,h", [(17, 9), (321, 183), (1920, 1080)])
def test_every_batch_position_gives_the_bytes_of_the_single_pair_call_and_of_a_second_run(nsc, w, h):
    n = 5
    a, b = _pairs(w, h, n)
    fb = w * h * 4
    da, db = put(a, "cuda:0"), put(b, "cuda:0")
    meas, cut = _detect(nsc, da.data_ptr(), fb, db.data_ptr(), fb, w, h, n)
    again = _detect(nsc, da.data_ptr(), fb, db.data_ptr(), fb, w, h, n)
    assert meas.tobytes() == again[0].tobytes() and cut.tobytes() == again[1].tobytes()
    for i in range(n):
        m1, c1 = _detect(nsc, da[i].data_ptr(), fb, db[i].data_ptr(), fb, w, h, 1)
        assert m1.tobytes() == meas[i:i + 1].tobytes() and c1[0] == cut[i], i


@pytest.mark.parametrize("w,h,pad", [(17, 9, 4), (321, 183, 260), (64, 32, 16)])
def test_padded_strides(nsc, w, h, pad):
    import torch

    n = 5
    a, b = _pairs(w, h, n)
    fb = w * h * 4
    da = torch.full((n, fb + pad), 0xEE, dtype=torch.uint8, device="cuda:0")
    db = torch.full((n, fb + 2 * pad), 0x11, dtype=torch.uint8, device="cuda:0")
    da[:, :fb] = put(a.reshape(n, fb), "cuda:0")
    db[:, :fb] = put(b.reshape(n, fb), "cuda:0")
    meas, cut = _detect(nsc, da.data_ptr(), fb + pad, db.data_ptr(), fb + 2 * pad, w, h, n)
    _assert_equal(meas, cut, *_want(a, b))


@pytest.mark.parametrize("w,h", [(17, 9), (320, 180)])
def test_sliding_stream(nsc, w, h):
    n = 7
    frames = np.stack([_frame(w, h, k) for k in range(n)])
    fb = w * h * 4
    d = put(frames, "cuda:0")
    meas, cut = _detect(nsc, d.data_ptr(), fb, d.data_ptr() + fb, fb, w, h, n - 1)
    _assert_equal(meas, cut, *_want(frames[:-1], frames[1:]))


@pytest.mark.parametrize("w,h", [(17, 9), (321, 183)])
def test_channel_orders(nsc, w, h):
    n = 5
    a, b = _pairs(w, h, n)
    fb = w * h * 4
    da, db = put(a, "cuda:0"), put(b, "cuda:0")
    got = {}
    for name, fmt in (("rgba", sc.RGBA), ("bgra", sc.BGRA), ("rgbx", sc.RGBX), ("bgrx", sc.BGRX)):
        meas, cut = _detect(nsc, da.data_ptr(), fb, db.data_ptr(), fb, w, h, n, fmt=name)
        _assert_equal(meas, cut, *_want(a, b, fmt))
        got[name] = meas.tobytes()
    assert got["rgba"] == got["rgbx"] and got["bgra"] == got["bgrx"] and got["rgba"] != got["bgra"]
    # BGRA gives the numbers of the swizzled RGBA
    sa, sb = np.ascontiguousarray(a[..., [2, 1, 0, 3]]), np.ascontiguousarray(b[..., [2, 1, 0, 3]])
    dsa, dsb = put(sa, "cuda:0"), put(sb, "cuda:0")
    meas, _ = _detect(nsc, dsa.data_ptr(), fb, dsb.data_ptr(), fb, w, h, n, fmt="bgra")
    assert meas.tobytes() == got["rgba"]


def test_decisions_on_content_with_wide_margins(nsc):
    w, h = 320, 180
    cases = decision_cases(w, h)
    a = np.stack([c[1] for c in cases])
    b = np.stack([c[2] for c in cases])
    fb = w * h * 4
    da, db = put(a, "cuda:0"), put(b, "cuda:0")
    meas, cut = _detect(nsc, da.data_ptr(), fb, db.data_ptr(), fb, w, h, len(cases))
    _assert_equal(meas, cut, *_want(a, b))
    assert cut.tolist() == [1 if c[3] else 0 for c in cases], [c[0] for c in cases]
    for name, x, y, want, _, _ in cases:
        got_cut, sad, hist = nsc.SceneDetector().detect(x, y, w, h)  # the host entry point, one pair
        assert (got_cut, (sad, hist)) == (want, sc.measures(x, y)), name


def test_host_entry_point_reuses_its_grown_buffers(nsc):
    """nus_scene_detect on one device with a 16x12 pair, a 48x32 pair (the kept buffers grow) and the 16x12 pair again (they are
    reused, larger than needed): each answer equals the yardstick's, so the third equals the first."""
    got = []
    for w, h in ((16, 12), (48, 32), (16, 12)):
        x, y = _frame(w, h, 0), _frame(w, h, 3)
        cut, sad, hist = nsc.SceneDetector().detect(x, y, w, h)
        s, l = sc.measures(x, y)
        assert (cut, (sad, hist)) == (sc.is_cut(s, l, w, h, 20, 400), (s, l)), (w, h)
        got.append((cut, sad, hist))
    assert got[2] == got[0]


def test_threshold_extremes(nsc):
    w, h = 64, 32
    n = 5
    a, b = _pairs(w, h, n)
    a, b = a.copy(), b.copy()
    b[0] = a[0]  # an identical pair: sad 0, hist 0
    a[1, ..., :3], b[1, ..., :3] = 0, 255  # black -> white: sad 255 * 3 W H, hist 2 W H exactly
    fb = w * h * 4
    da, db = put(a, "cuda:0"), put(b, "cuda:0")
    for mad, hist in ((0, 0), (255, 1000), (255, 0), (0, 1000), (1, 1)):
        meas, cut = _detect(nsc, da.data_ptr(), fb, db.data_ptr(), fb, w, h, n, mad=mad, hist=hist)
        want_m, want_c = _want(a, b, mad=mad, hist=hist)
        _assert_equal(meas, cut, want_m, want_c)
        if (mad, hist) == (0, 0):
            assert want_c == [1] * n
        if (mad, hist) == (255, 1000):
            assert want_c == [0, 1, 0, 0, 0] and want_m[1] == (255 * 3 * w * h, 2 * w * h)


def test_non_default_stream(nsc):
    import torch

    w, h, n = 321, 183, 5
    a, b = _pairs(w, h, n)
    fb = w * h * 4
    da, db = put(a, "cuda:0"), put(b, "cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        meas, cut = _detect(nsc, da.data_ptr(), fb, db.data_ptr(), fb, w, h, n, stream=s.cuda_stream)
    _assert_equal(meas, cut, *_want(a, b))


TIME_SETS = [[0.0, 0.5, 1.0], frame_times(8), [0.25], [0.49999997, 0.5, 0.50000006, 0.0, 1.0, 0.75, 0.125]]


APPLY_CASES = [(w, h, t, "rgba") for w, h in [(1, 1), (17, 9), (64, 32), (321, 183)] for t in range(len(TIME_SETS))] + \
              [(w, h, 0, f) for w, h in [(17, 9), (64, 32), (321, 183)] for f in ("bgra", "bgrx")]  # the channel orders at one time set


@pytest.mark.parametrize("w,h,time_set,fmt", APPLY_CASES)
def test_apply_overwrites_cut_pairs_only(nsc, w, h, time_set, fmt):
    import torch

    times = TIME_SETS[time_set]
    n, nt = 5, len(times)
    a, b = _pairs(w, h, n)
    fb = w * h * 4
    flags = [1, 0, 1, 1, 0]
    da, db, dc = put(a, "cuda:0"), put(b, "cuda:0"), put(np.array(flags, np.uint8), "cuda:0")
    code = {"rgba": sc.RGBA, "bgra": sc.BGRA, "bgrx": sc.BGRX}[fmt]
    for gap in (0, 1):  # tightly packed, and a display-order stride whose gap frame must stay untouched
        out = guarded.empty((n, nt + gap, h, w, 4), dtype=torch.uint8, device="cuda:0")
        nsc.SceneDetector().apply_cuts_device(da.data_ptr(), fb, db.data_ptr(), fb, w, h, times, dc.data_ptr(), out.data_ptr(),
                                              (nt + gap) * fb if gap else 0, n, fmt, _stream())
        want = np.full((n, nt + gap, h, w, 4), POISON, np.uint8)
        sc.apply_cuts(a, b, flags, times, want[:, :nt], code)
        assert np.array_equal(fetch(out), want)


def test_apply_with_padded_unequal_input_strides(nsc):
    import torch

    w, h, n, pad = 17, 9, 5, 20
    a, b = _pairs(w, h, n)
    fb = w * h * 4
    times, flags = [0.25, 0.5, 0.75], [0, 1, 1, 0, 1]
    da = torch.full((n, fb + pad), 0xEE, dtype=torch.uint8, device="cuda:0")
    db = torch.full((n, fb + 3 * pad), 0x11, dtype=torch.uint8, device="cuda:0")
    da[:, :fb] = put(a.reshape(n, fb), "cuda:0")
    db[:, :fb] = put(b.reshape(n, fb), "cuda:0")
    dc = put(np.array(flags, np.uint8), "cuda:0")
    out = guarded.empty((n, 4, h, w, 4), dtype=torch.uint8, device="cuda:0")
    nsc.SceneDetector().apply_cuts_device(da.data_ptr(), fb + pad, db.data_ptr(), fb + 3 * pad, w, h, times, dc.data_ptr(), out.data_ptr(),
                                          4 * fb, n, "rgba", _stream())
    want = np.full((n, 4, h, w, 4), POISON, np.uint8)
    sc.apply_cuts(a, b, flags, times, want[:, :3])
    assert np.array_equal(fetch(out), want)


def test_apply_equals_the_zero_flow_interpolation_at_the_ends(nsc):
    """The rule's "copy" is by definition what nus_interp_interpolate_device writes at t = 0 and t = 1 for the input format."""
    import torch

    w, h, n = 64, 32, 5
    a, b = _pairs(w, h, n)
    fb = w * h * 4
    da, db, dc = put(a, "cuda:0"), put(b, "cuda:0"), put(np.ones(n, np.uint8), "cuda:0")
    for fmt in ("rgba", "bgra", "rgbx", "bgrx"):
        it = nsc.WgpuFrameInterpolator()
        it.set_input_format(fmt)
        ends = guarded.empty((n, 2, h, w, 4), dtype=torch.uint8, device="cuda:0")
        it.interpolate_multi_device(da.data_ptr(), fb, db.data_ptr(), fb, 0, w, h, [0.0, 1.0], ends.data_ptr(), 0, n, _stream())
        out = guarded.empty((n, 2, h, w, 4), dtype=torch.uint8, device="cuda:0")
        nsc.SceneDetector().apply_cuts_device(da.data_ptr(), fb, db.data_ptr(), fb, w, h, [0.25, 0.75], dc.data_ptr(), out.data_ptr(), 0, n,
                                              fmt, _stream())
        assert np.array_equal(fetch(out), fetch(ends)), fmt


def _cut_stream(w, h):
    """12 frames, cuts after frames 3 and 8: three shots of slowly panning content."""
    shots = [lambda k: sine_pattern(w, h, 1.0 * k), lambda k: gradient_frame(w, h, k), lambda k: (sine_pattern(w, h, 0.5 * k) // 3)]
    frames = []
    for k in range(12):
        f = np.ascontiguousarray(shots[0 if k <= 3 else 1 if k <= 8 else 2](k)).copy()
        f[..., 3] = 255
        frames.append(f)
    return np.stack(frames)


def test_detection_off_is_the_default_and_changes_nothing(nsc):
    import torch

    w, h = 96, 64
    frames = _cut_stream(w, h)
    times = frame_times(4)
    d = put(frames, "cuda:0")
    outs = []
    for touch in (False, True):
        fl = nsc.FlowEstimator()
        if touch:
            fl.set_scene_detect(True)
            fl.set_scene_detect(False)
        mid = guarded.empty((11, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
        fl.interpolate_multi_device_stream(d.data_ptr(), 12, w, h, times, mid.data_ptr(), stream=_stream())
        outs.append(fetch(mid))
    assert np.array_equal(outs[0], outs[1])
    bm0, bm1 = nsc.BlockMatcher(), nsc.BlockMatcher()
    plain = bm0.interpolate(frames[3], frames[4], w, h, times=times)
    repeats = [frames[3].tobytes(), frames[4].tobytes(), frames[4].tobytes()]
    assert plain != repeats
    bm1.set_scene_detect(True)
    bm1.set_scene_detect(False)
    assert bm1.interpolate(frames[3], frames[4], w, h, times=times) == plain
    # the per-call flag holds for its call only, with the thresholds the object was given
    assert bm1.interpolate(frames[3], frames[4], w, h, times=times, scene_detect=True) == repeats
    assert bm1.scene_detect is False and bm1.interpolate(frames[3], frames[4], w, h, times=times) == plain
    bm1.set_scene_detect(False, 255, 1000)
    assert bm1.interpolate(frames[3], frames[4], w, h, times=times, scene_detect=True) == plain
    bm1.set_scene_detect(True)
    assert bm1.interpolate(frames[3], frames[4], w, h, times=times) == repeats


@pytest.mark.parametrize("w,h", [(96, 64), (321, 183)])
def test_end_to_end_stream_with_two_cuts(nsc, w, h):
    import torch

    frames = _cut_stream(w, h)
    times = frame_times(4)
    want_cut = [1 if sc.is_cut(*sc.measures(frames[k], frames[k + 1]), w, h) else 0 for k in range(11)]
    assert want_cut == [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]
    d = put(frames, "cuda:0")
    # optical flow: one device stream call
    res = {}
    for on in (False, True):
        fl = nsc.FlowEstimator()
        fl.set_scene_detect(on)
        mid = guarded.empty((11, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
        fl.interpolate_multi_device_stream(d.data_ptr(), 12, w, h, times, mid.data_ptr(), stream=_stream())
        res[on] = fetch(mid)
    want = res[False].copy()
    sc.apply_cuts(frames[:-1], frames[1:], want_cut, times, want)
    assert np.array_equal(res[True], want)
    for k in (3, 8):
        assert np.array_equal(res[True][k, 0], frames[k]) and np.array_equal(res[True][k, 1], frames[k + 1])
        assert np.array_equal(res[True][k, 2], frames[k + 1]) and not np.array_equal(res[False][k], res[True][k])
    # block matching: the host pair entry point, pair by pair
    plain, aware = nsc.BlockMatcher(), nsc.BlockMatcher()
    for k in range(11):
        base = plain.interpolate(frames[k], frames[k + 1], w, h, times=times)
        got = aware.interpolate(frames[k], frames[k + 1], w, h, times=times, scene_detect=True)
        if want_cut[k]:
            assert got == [frames[k].tobytes(), frames[k + 1].tobytes(), frames[k + 1].tobytes()], k
        else:
            assert got == base, k
    # the Python-level paths: multi-time zero-flow / given-flow interpolation and the pyclass
    it = nsc.WgpuFrameInterpolator()
    for k in (2, 3):
        base = it.interpolate_multi_py(frames[k], frames[k + 1], w, h, times=times)
        got = it.interpolate_multi_py(frames[k], frames[k + 1], w, h, times=times, scene_detect=True)
        assert got == ([frames[k].tobytes(), frames[k + 1].tobytes(), frames[k + 1].tobytes()] if want_cut[k] else base), k
    for method in ("optical_flow", "block_matching"):
        py0, py1 = nsc.PyFrameInterpolator(method), nsc.PyFrameInterpolator(method, scene_detect=True)
        py0.initialize(w, h)
        py1.initialize(w, h)
        assert py1.interpolate(frames[3], frames[4], 0.25) == frames[3].tobytes()
        assert py1.interpolate(frames[3], frames[4], 0.5) == frames[4].tobytes()
        assert py1.interpolate(frames[1], frames[2], 0.25) == py0.interpolate(frames[1], frames[2], 0.25)


def test_both_clis_print_the_library_verdict(nsc, tmp_path):
    import os
    import subprocess
    import sys

    from conftest import ROOT
    from nu_scaler_amd.imagefile import write_png

    w, h = 64, 48
    a, b = sine_pattern(w, h), gradient_frame(w, h)
    pa, pb = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    write_png(pa, w, h, a.tobytes())
    write_png(pb, w, h, b.tobytes())
    cut, sad, hist = nsc.SceneDetector().detect(a, b, w, h)
    assert (cut, (sad, hist)) == (sc.is_cut(*sc.measures(a, b), w, h), sc.measures(a, b))
    from nu_scaler_amd.cli import scene_line

    line = scene_line(cut, sad, hist, w, h)
    env = dict(os.environ, PYTHONPATH=ROOT)
    py = subprocess.run([sys.executable, "-m", "nu_scaler_amd.cli", "scene", pa, pb], capture_output=True, text=True, env=env, timeout=300)
    assert py.returncode == 0 and py.stdout.strip() == line, (py.stdout, py.stderr)
    exe = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    nat = subprocess.run([exe, "scene", pa, pb], capture_output=True, text=True, timeout=300)
    assert nat.returncode == 0 and nat.stdout.strip() == line, (nat.stdout, nat.stderr)
    # --scene-detect: both tools write the repeats for this pair (a cut), byte for byte
    from _png import read_png

    for tool, argv in (("py", [sys.executable, "-m", "nu_scaler_amd.cli"]), ("native", [exe])):
        out = str(tmp_path / f"{tool}.png")
        r = subprocess.run(argv + ["interpolate", pa, pb, out, "--multiplier", "3", "--scene-detect"], capture_output=True, text=True,
                           env=env, timeout=300)
        assert r.returncode == 0, (r.stdout, r.stderr)
        stem = str(tmp_path / tool)
        assert np.array_equal(read_png(stem + "_1.png"), a) == bool(cut) and np.array_equal(read_png(stem + "_2.png"), b) == bool(cut)
