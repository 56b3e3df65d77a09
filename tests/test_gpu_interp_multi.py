"""Several in-between frames per pair from one launch, on the MI355X: nus_interp_interpolate_multi_device,
nus_interp_interpolate_multi and nus_flow_interpolate_multi_device_stream write, for every time of the set, the bytes the
single-time entry point writes at that time -- every mode, flow format and input format, the vector and the scalar zero-flow
kernels, the dense kernel's 2 x 2 and 1 x 2 shapes and the tiny-frame kernel.  Every device output comes from conftest.guarded."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu


def _f32(ts):
    return [float(np.float32(t)) for t in ts]


TIME_SETS = [_f32([0.5]), _f32([1 / 3, 2 / 3]), _f32([0.25, 0.5, 0.75]), _f32([k / 8 for k in range(1, 8)]),
             _f32([0.0, 1.0, 0.3, 0.3, 0.7])]  # K = 1, 2, 3, 7 and an irregular set with both ends and a duplicate
SIZES = [(1920, 1080), (333, 117), (1, 37), (37, 1)]


def _frames(n, w, h, seed):
    return np.random.default_rng(seed + 31 * w + h).integers(0, 256, (n, h, w, 4), dtype=np.uint8)


def _smooth_flow(n, w, h, seed, amp=4.0):
    """Smooth random flows of about `amp` pixels."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((n, h, w, 2), np.float32)
    for i in range(n):
        p, f = rng.uniform(0, 2 * np.pi, 4), rng.uniform(17, 61, 4)
        out[i, ..., 0] = amp * np.sin(x / f[0] + p[0]) * np.cos(y / f[1] + p[1])
        out[i, ..., 1] = amp * np.cos(x / f[2] + p[2]) * np.sin(y / f[3] + p[3])
    return out


def _smooth_frame(w, h, shift=0.0):
    x = np.arange(w, dtype=np.float64)[None, :] - shift
    y = np.arange(h, dtype=np.float64)[:, None]
    v = 127.5 + 45 * np.sin(x / 3.0) * np.cos(y / 4.0) + 50 * np.sin((x + 2 * y) / 23.0) + 25 * np.sin(x / 9.0 + y / 11.0)
    img = np.empty((h, w, 4), np.uint8)
    img[..., 0] = np.clip(v, 0, 255)
    img[..., 1] = np.clip(255 - v, 0, 255)
    img[..., 2] = np.clip(v * 0.5 + 40, 0, 255)
    img[..., 3] = 255
    return img


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _single(it, d_frames, d_flow, w, h, t, n_pairs):
    """n_pairs in-between frames of the sliding stream at t, from the single-time entry point."""
    import torch

    fb = w * h * 4
    out = guarded.empty((n_pairs, h, w, 4), dtype=torch.uint8, device="cuda:0")
    it.interpolate_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_flow.data_ptr() if d_flow is not None else 0,
                          w, h, t, out.data_ptr(), n_pairs, _stream())
    return fetch(out)


def _multi(it, d_frames, d_flow, w, h, times, n_pairs):
    import torch

    fb = w * h * 4
    out = guarded.empty((n_pairs, len(times), h, w, 4), dtype=torch.uint8, device="cuda:0")
    it.interpolate_multi_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_flow.data_ptr() if d_flow is not None else 0,
                                w, h, times, out.data_ptr(), 0, n_pairs, _stream())
    return fetch(out)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", ["rgba", "bgra", "rgbx", "bgrx"])
def test_zero_flow_frames_equal_single_time_calls(nsc, oracle_mod, w, h, fmt):
    n_pairs = 3
    frames = _frames(n_pairs + 1, w, h, 1)
    d_frames = put(frames)
    it = nsc.WgpuFrameInterpolator()
    it.set_input_format(fmt)
    for times in TIME_SETS:
        got = _multi(it, d_frames, None, w, h, times, n_pairs)
        for k, t in enumerate(times):
            assert np.array_equal(got[:, k], _single(it, d_frames, None, w, h, t, n_pairs)), (fmt, w, h, times, k)
            if fmt == "rgba":
                for i in range(n_pairs):
                    assert np.array_equal(got[i, k], oracle_mod.warp_blend(frames[i], frames[i + 1], None, t)), (w, h, times, k, i)


@pytest.mark.parametrize("w,h", SIZES + [(334, 117)])
@pytest.mark.parametrize("mode,ffmt", [("exact", "f32"), ("fma", "f32"), ("exact", "f16"), ("fma", "f16")])
def test_dense_flow_frames_equal_single_time_calls(nsc, oracle_mod, w, h, mode, ffmt):
    n_pairs = 3
    frames = _frames(n_pairs + 1, w, h, 2)
    flow = _smooth_flow(n_pairs, w, h, 3)
    d_frames = put(frames)
    d_flow = put(flow if ffmt == "f32" else flow.astype(np.float16))
    it = nsc.WgpuFrameInterpolator()
    it.set_mode(mode)
    it.set_flow_format(ffmt)
    for times in TIME_SETS:
        got = _multi(it, d_frames, d_flow, w, h, times, n_pairs)
        for k, t in enumerate(times):
            assert np.array_equal(got[:, k], _single(it, d_frames, d_flow, w, h, t, n_pairs)), (mode, ffmt, w, h, times, k)
            if mode == "exact" and ffmt == "f32" and len(times) <= 5:
                for i in range(n_pairs):
                    assert np.array_equal(got[i, k], oracle_mod.warp_blend(frames[i], frames[i + 1], flow[i], t)), (w, h, times, k, i)


@pytest.mark.parametrize("w,h", [(1920, 1080), (333, 117), (37, 1)])
@pytest.mark.parametrize("with_flow", [False, True])
def test_display_order_stride_leaves_the_gaps_alone(nsc, w, h, with_flow):
    """Pair stride (K + 1) frames, output from frame 1 on: the caller's real frame goes into each gap, which the call must not touch."""
    import torch

    n_pairs, times = 3, _f32([0.25, 0.5, 0.75])
    K, fb = len(times), w * h * 4
    d_frames = put(_frames(n_pairs + 1, w, h, 4))
    d_flow = put(_smooth_flow(n_pairs, w, h, 5)) if with_flow else None
    it = nsc.WgpuFrameInterpolator()
    it.set_mode("fma")
    buf = guarded.full((n_pairs * (K + 1) * fb,), 0x5A, dtype=torch.uint8, device="cuda:0")
    it.interpolate_multi_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_flow.data_ptr() if with_flow else 0, w, h, times,
                                buf.data_ptr() + fb, (K + 1) * fb, n_pairs, _stream())
    got = fetch(buf).reshape(n_pairs, K + 1, h, w, 4)
    assert bool((got[:, 0] == 0x5A).all())
    for k, t in enumerate(times):
        assert np.array_equal(got[:, k + 1], _single(it, d_frames, d_flow, w, h, t, n_pairs)), (w, h, k)


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("with_flow", [False, True])
def test_host_entry_equals_single_time_host_calls(nsc, pinned, with_flow):
    w, h = 640, 360
    fb = w * h * 4
    a, b = _frames(2, w, h, 6)
    flow = _smooth_flow(1, w, h, 7)[0] if with_flow else None
    times = _f32([0.2, 0.4, 0.6, 0.8, 0.5])
    lib = nsc._capi.lib()
    it = nsc.WgpuFrameInterpolator()
    for mode in ("exact", "fma"):
        it.set_mode(mode)
        want = [it.interpolate_py(a, b, w, h, time_t=t, flow=flow) for t in times]
        out = np.full(len(times) * fb, 0x33, np.uint8)
        pin = nsc.PinnedBuffer(out) if pinned else None
        ts = (ctypes.c_float * len(times))(*times)
        st = lib.nus_interp_interpolate_multi(it._h, a.ctypes.data, fb, b.ctypes.data, fb, flow.ctypes.data if with_flow else None, w, h,
                                              ts, len(times), out.ctypes.data, out.nbytes)
        if pin is not None:
            pin.unpin()
        assert st == nsc._capi.OK, it._err()
        for k in range(len(times)):
            assert out[k * fb:(k + 1) * fb].tobytes() == want[k], (mode, k)
        ms = it.get_last_gpu_duration_ms()
        assert ms is not None and ms > 0.0


@pytest.mark.parametrize("w,h", [(320, 184), (1920, 1080)])
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("fmode", ["exact", "fast"])
def test_motion_stream_estimates_once_and_matches_single_calls(nsc, w, h, ffmt, fmode):
    import torch

    n_frames, times = 4, _f32([0.25, 0.5, 0.75])
    K, n_pairs, fb = len(times), n_frames - 1, w * h * 4
    d_frames = put(np.stack([_smooth_frame(w, h, 1.3 * k) for k in range(n_frames)]))
    fdt = torch.float32 if ffmt == "f32" else torch.float16
    fe = nsc.FlowEstimator()
    fe.set_mode(fmode)
    s = _stream()
    want_mid, want_flows = [], None
    for t in times:
        mid = guarded.empty((n_pairs, h, w, 4), dtype=torch.uint8, device="cuda:0")
        flows = guarded.empty((n_pairs, h, w, 2), dtype=fdt, device="cuda:0")
        fe.interpolate_device_stream(d_frames.data_ptr(), n_frames, w, h, t, mid.data_ptr(), flows.data_ptr(), s, flow_format=ffmt)
        want_mid.append(fetch(mid))
        f = fetch(flows).view(np.uint8)
        assert want_flows is None or np.array_equal(f, want_flows)  # the flows do not depend on t
        want_flows = f
    for with_flows in (True, False):
        mid = guarded.empty((n_pairs, K, h, w, 4), dtype=torch.uint8, device="cuda:0")
        flows = guarded.empty((n_pairs, h, w, 2), dtype=fdt, device="cuda:0") if with_flows else None
        fe.interpolate_multi_device_stream(d_frames.data_ptr(), n_frames, w, h, times, mid.data_ptr(),
                                           flows.data_ptr() if with_flows else 0, 0, s, flow_format=ffmt)
        got = fetch(mid)
        for k in range(K):
            assert np.array_equal(got[:, k], want_mid[k]), (ffmt, fmode, with_flows, k)
        if with_flows:
            assert np.array_equal(fetch(flows).view(np.uint8), want_flows)
    # display order: pair stride K + 1 frames, the gaps untouched
    buf = guarded.full((n_pairs * (K + 1) * fb,), 0x5A, dtype=torch.uint8, device="cuda:0")
    fe.interpolate_multi_device_stream(d_frames.data_ptr(), n_frames, w, h, times, buf.data_ptr() + fb, 0, (K + 1) * fb, s,
                                       flow_format=ffmt)
    got = fetch(buf).reshape(n_pairs, K + 1, h, w, 4)
    assert bool((got[:, 0] == 0x5A).all())
    for k in range(K):
        assert np.array_equal(got[:, k + 1], want_mid[k])


def _write_png(path, img):
    from nu_scaler_amd.imagefile import write_png

    write_png(str(path), img.shape[1], img.shape[0], np.ascontiguousarray(img).tobytes())


def test_interpolate_multi_py_and_both_clis(nsc, tmp_path):
    from nu_scaler_amd.imagefile import read_png

    w, h = 160, 96
    a, b = _smooth_frame(w, h), _smooth_frame(w, h, 1.5)
    it = nsc.WgpuFrameInterpolator()
    got = it.interpolate_multi_py(a, b, w, h, multiplier=4)
    assert got == [it.interpolate_py(a, b, w, h, time_t=t) for t in (0.25, 0.5, 0.75)]
    _write_png(tmp_path / "a.png", a)
    _write_png(tmp_path / "b.png", b)
    native = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    assert os.path.exists(native)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for name, cmd in (("native", [native]), ("py", [sys.executable, "-m", "nu_scaler_amd.cli"])):
        for flow in ([], ["--flow"]):
            tag = f"{name}{'_flow' if flow else ''}"
            base = [*cmd, "interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png")]
            r = subprocess.run(base + [str(tmp_path / f"{tag}_m.png"), "--multiplier", "4"] + flow, capture_output=True, text=True,
                               timeout=300, cwd=ROOT, env=env)
            assert r.returncode == 0, r.stderr
            for k, t in enumerate(("0.25", "0.5", "0.75"), 1):
                r = subprocess.run(base + [str(tmp_path / f"{tag}_t{k}.png"), "--t", t] + flow, capture_output=True, text=True,
                                   timeout=300, cwd=ROOT, env=env)
                assert r.returncode == 0, r.stderr
                m = open(tmp_path / f"{tag}_m_{k}.png", "rb").read()
                assert m == open(tmp_path / f"{tag}_t{k}.png", "rb").read(), (tag, k)
                if not flow:
                    assert read_png(str(tmp_path / f"{tag}_m_{k}.png"))[2] == got[k - 1], (tag, k)
            assert not os.path.exists(tmp_path / f"{tag}_m_4.png") and not os.path.exists(tmp_path / f"{tag}_m.png")
