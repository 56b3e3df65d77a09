"""Scene-cut detector: what can be checked without a device -- the argument validation of the C entry points (every error is
returned before any HIP call, with a text naming the entry point), the Python surface and the CLI's argument parsing."""
import ctypes

import numpy as np
import pytest

from nu_scaler_amd import _capi as C

W, H = 16, 8
FB = W * H * 4
A, B, WS, CUT, OUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # never dereferenced: the checks fail first


def _times(*ts):
    return (ctypes.c_float * len(ts))(*ts)


def _detect(lib, **kw):
    a = dict(d_a=A, a_stride=FB, d_b=B, b_stride=FB, w=W, h=H, n=1, fmt=0, mad=20, hist=400, ws=WS, ws_bytes=1 << 20, meas=None, cut=CUT)
    a.update(kw)
    return lib.nus_scene_detect_device(a["d_a"], a["a_stride"], a["d_b"], a["b_stride"], a["w"], a["h"], a["n"], a["fmt"], a["mad"],
                                       a["hist"], a["ws"], a["ws_bytes"], a["meas"], a["cut"], None)


def _apply(lib, **kw):
    a = dict(d_a=A, a_stride=FB, d_b=B, b_stride=FB, w=W, h=H, fmt=0, times=_times(0.25, 0.5), n_times=2, cut=CUT, out=OUT, stride=0, n=1)
    a.update(kw)
    return lib.nus_scene_apply_cuts_device(a["d_a"], a["a_stride"], a["d_b"], a["b_stride"], a["w"], a["h"], a["fmt"], a["times"],
                                           a["n_times"], a["cut"], a["out"], a["stride"], a["n"], None)


def test_abi_version_is_unchanged(nsc):
    assert C.lib().nus_abi_version() == 1


def test_workspace_size(nsc):
    lib = C.lib()
    one = lib.nus_scene_workspace_size(1920, 1080, 1)
    assert one > 0 and one % 8 == 0
    assert lib.nus_scene_workspace_size(1920, 1080, 32) == 32 * one
    assert lib.nus_scene_workspace_size(1920, 1080, 0) == one
    assert lib.nus_scene_workspace_size(1, 1, 1) > 0
    for w, h in ((0, 8), (8, 0), (1 << 16, 1 << 15)):
        assert lib.nus_scene_workspace_size(w, h, 1) == 0
        assert "nus_scene_workspace_size" in C.last_error()


@pytest.mark.parametrize("kw", [
    dict(d_a=None), dict(d_b=None), dict(ws=None), dict(cut=None), dict(w=0), dict(h=0), dict(fmt=4), dict(fmt=-1), dict(mad=256),
    dict(hist=1001), dict(d_a=A + 2), dict(d_b=B + 1), dict(a_stride=FB + 2), dict(b_stride=FB - 4), dict(a_stride=0), dict(ws=WS + 4),
    dict(meas=0x60004), dict(ws_bytes=8), dict(n=0, mad=300), dict(n=0, b_stride=4),
])
def test_detect_device_argument_errors(nsc, kw):
    assert _detect(C.lib(), **kw) == C.ERR_INVALID_ARGUMENT
    assert "nus_scene_detect_device" in C.last_error()


def test_zero_pairs_is_ok_without_a_device(nsc):
    lib = C.lib()
    assert _detect(lib, n=0) == C.OK
    assert _apply(lib, n=0) == C.OK


@pytest.mark.parametrize("kw", [
    dict(d_a=None), dict(d_b=None), dict(cut=None), dict(out=None), dict(w=0), dict(fmt=7), dict(times=None), dict(n_times=0),
    dict(n_times=8, times=_times(*[0.5] * 8)), dict(times=_times(0.25, 1.5)), dict(times=_times(float("nan"), 0.5)),
    dict(times=_times(-0.1, 0.5)), dict(out=OUT + 2), dict(stride=2 * FB - 4), dict(stride=2 * FB + 2), dict(a_stride=FB - 4),
    dict(d_b=B + 3), dict(n=0, n_times=0),
])
def test_apply_argument_errors(nsc, kw):
    assert _apply(C.lib(), **kw) == C.ERR_INVALID_ARGUMENT
    assert "nus_scene_apply_cuts_device" in C.last_error()


def test_host_entry_point_argument_errors(nsc):
    lib = C.lib()
    a = np.zeros(FB, np.uint8)
    cut = ctypes.c_uint8(7)
    call = lambda **kw: lib.nus_scene_detect(kw.get("device", 0), kw.get("a", a.ctypes.data), kw.get("a_len", FB), kw.get("b", a.ctypes.data),
                                             kw.get("b_len", FB), kw.get("w", W), kw.get("h", H), kw.get("fmt", 0), kw.get("mad", 20),
                                             kw.get("hist", 400), None, kw.get("cut", ctypes.addressof(cut)))
    for kw in (dict(a=None), dict(b=None), dict(cut=None), dict(w=0), dict(fmt=9), dict(mad=256), dict(hist=2000)):
        assert call(**kw) == C.ERR_INVALID_ARGUMENT, kw
        assert "nus_scene_detect" in C.last_error()
    assert call(b_len=FB - 4) == C.ERR_SIZE_MISMATCH and C.last_error() == "Images must have the same dimensions"
    assert call(a_len=FB - 4, b_len=FB - 4) == C.ERR_SIZE_MISMATCH and "does not match expected input buffer size" in C.last_error()
    assert cut.value == 7


def test_handle_setters(nsc):
    lib = C.lib()
    for create, destroy, setter, err in ((lib.nus_flow_create, lib.nus_flow_destroy, lib.nus_flow_set_scene_detect, lib.nus_flow_last_error),
                                         (lib.nus_bm_create, lib.nus_bm_destroy, lib.nus_bm_set_scene_detect, lib.nus_bm_last_error)):
        h = create()
        try:
            assert setter(h, 1, 20, 400) == C.OK and setter(h, 0, 0, 0) == C.OK and setter(h, 1, 255, 1000) == C.OK
            for bad in ((2, 20, 400), (1, 256, 400), (1, 20, 1001)):
                assert setter(h, *bad) == C.ERR_INVALID_ARGUMENT
                assert b"set_scene_detect" in err(h)
        finally:
            destroy(h)
        assert setter(None, 1, 20, 400) == C.ERR_INVALID_ARGUMENT


def test_python_surface(nsc):
    from nu_scaler_amd.scene import MEASURES_DTYPE, check_thresholds, pixel_format

    det = nsc.SceneDetector()
    assert (det.mad_threshold, det.hist_permille, det.device) == (20, 400, 0)
    assert nsc.SceneDetector(0, 1000, device=0).hist_permille == 1000
    assert MEASURES_DTYPE.itemsize == 16
    for bad in ((-1, 400), (256, 400), (20, 1001), (20.5, 400), (True, 400)):
        with pytest.raises(ValueError):
            nsc.SceneDetector(*bad)
        with pytest.raises(ValueError):
            check_thresholds(*bad)
    assert [pixel_format(f) for f in ("rgba", "BGRA", "rgbx", "bgrx", 1)] == [0, 1, 2, 3, 1]
    with pytest.raises(ValueError):
        pixel_format("argb")
    assert nsc.SceneDetector.workspace_size(1920, 1080, 4) == C.lib().nus_scene_workspace_size(1920, 1080, 4)
    with pytest.raises(ValueError):
        nsc.SceneDetector.workspace_size(0, 4)
    with pytest.raises(ValueError, match="nus_scene_detect_device"):
        det.detect_device(A, FB, B, FB - 4, W, H, 1, WS, 1 << 20, CUT)
    with pytest.raises(ValueError, match="nus_scene_apply_cuts_device"):
        det.apply_cuts_device(A, FB, B, FB, W, H, [0.5, 2.0], CUT, OUT)
    with pytest.raises(ValueError):  # size mismatch of a host pair, before any device is asked for
        det.detect(bytes(FB), bytes(FB - 4), W, H)
    bm = nsc.BlockMatcher()
    assert bm.scene_detect is False
    bm.set_scene_detect(True, 30, 500)
    assert bm.scene_detect is True
    with pytest.raises(ValueError):
        bm.set_scene_detect(True, 300)
    fl = nsc.FlowEstimator()
    fl.set_scene_detect(True)
    with pytest.raises(ValueError):
        fl.set_scene_detect(True, 20, 1001)
    import inspect

    assert inspect.signature(nsc.WgpuFrameInterpolator.interpolate_multi_py).parameters["scene_detect"].default is False
    assert inspect.signature(nsc.PyFrameInterpolator.__init__).parameters["scene_detect"].default is False
    assert inspect.signature(nsc.interpolate_image_files_multi).parameters["scene_detect"].default is False
    assert inspect.signature(nsc.BlockMatcher.interpolate).parameters["scene_detect"].default is False
    assert nsc.PyFrameInterpolator("block_matching", scene_detect=True)._scene is None
    assert nsc.PyFrameInterpolator("block_matching", scene_detect=True)._bm.scene_detect is True
    assert nsc.PyFrameInterpolator("optical_flow", scene_detect=True)._scene is not None
    assert nsc.PyFrameInterpolator("optical_flow")._scene is None


def test_cli_parsing(nsc, capsys):
    from nu_scaler_amd import cli

    p = cli.build_parser()
    a = p.parse_args(["scene", "a.png", "b.png"])
    assert (a.command, a.mad, a.hist, a.device) == ("scene", 20, 400, 0)
    a = p.parse_args(["scene", "a.png", "b.png", "--mad", "3", "--hist", "900", "--device", "1"])
    assert (a.mad, a.hist, a.device) == (3, 900, 1)
    assert p.parse_args(["interpolate", "a", "b", "o", "--multiplier", "4", "--scene-detect"]).scene_detect is True
    assert p.parse_args(["interpolate", "a", "b", "o", "--multiplier", "4"]).scene_detect is False
    for argv in (["scene", "a.png", "b.png", "--mad", "256"], ["scene", "a.png", "b.png", "--hist", "-1"],
                 ["interpolate", "a", "b", "o", "--scene-detect"], ["scene", "a.png"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
    assert cli.scene_line(True, 3 * 64 * 10, 64, 8, 8) == "cut=1 mad=10.000 hist_permille=500.0"
