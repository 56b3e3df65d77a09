"""nus_flow_set_warps on the GPU: the two host primitives against their numpy float32 restatement (tests/_flow_warp64.py), the EXACT
estimator against the composition of the primitives, EXACT and FAST against the float64 witness, the stream entry points against
the pair entry point and the warp, warps = 0 after warps = 1 against a fresh handle, and what the mode is for: the in-between
frame on scenes with a known true mid-frame.  Every device output comes from conftest.guarded."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _bm_bidir as scenes
import _flow_warp64 as W
import _scenecut as sc
from conftest import ROOT, guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

P = W.PARAMS  # levels 3, 50 + 10 steps, lambda 4e-4: the table's settings (and FlowEstimator's defaults)
FAST_CONTRACT = 1e-3  # px, nus_flow_set_mode(NUS_FLOW_FAST)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _estimator(nsc, warps=0, mode="exact", tiled=1):
    fe = nsc.FlowEstimator(P["levels"], P["coarse_iters"], P["refine_iters"], P["lam"], warps=warps)
    fe.set_mode(mode)
    fe.set_tiled(tiled)
    return fe


def _pair(size):
    """(a, b) RGBA8: 67 x 45 is the top-left crop of the table's first scene, 200 x 72 its fourth scene."""
    if size == (67, 45):
        a, b, _ = W.scene(W.ROWS[0])
        return np.ascontiguousarray(a[:45, :67]), np.ascontiguousarray(b[:45, :67])
    assert size == (200, 72)
    return W.scene(W.ROWS[3])[:2]


def _sequence(w, h, n, pan=(1, 0), mv=(2, 1), sq=24, seed=3):
    """n frames of _bm_bidir.scene's kind: the background pans by `pan` per frame, the square moves by `mv` per frame."""
    rng = np.random.default_rng(seed)
    M = 16
    bg = scenes.smooth_noise(rng, h + 2 * M, w + 2 * M)
    fg = scenes.smooth_noise(rng, sq, sq, 1)
    out = []
    for k in range(n):
        im = bg[M + pan[1] * k:M + pan[1] * k + h, M + pan[0] * k:M + pan[0] * k + w].copy()
        x0, y0 = 10 + mv[0] * k, 8 + mv[1] * k
        im[y0:y0 + sq, x0:x0 + sq] = fg
        out.append(np.dstack([im, np.full((h, w), 255, np.uint8)]))
    return np.stack(out)


_witness_cache = {}


def _witness(size, warps):
    """The float64 estimate of _pair(size), computed once per module run."""
    if (size, warps) not in _witness_cache:
        a, b = _pair(size)
        _witness_cache[size, warps] = W.estimate(a, b, warps=warps, **P)
    return _witness_cache[size, warps]


# ---- the host primitives ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (5, 3), (67, 45), (130, 70)])  # 67 and 130 cross the 64-lane strip once and twice
def test_warp_coefficients_equal_the_float32_restatement(nsc, w, h):
    rng = np.random.default_rng(100 * w + h)
    i1, i2 = rng.random((h, w, 4), np.float32), rng.random((h, w, 4), np.float32)
    fe = nsc.FlowEstimator()
    none = fe.warp_coefficients(i1, i2, None)
    assert np.array_equal(none, W.coefficients_f32(i1, i2, None))
    assert np.array_equal(none[..., 2], W.luminance_f32(i2) - W.luminance_f32(i1))
    flows = [((rng.random((h, w, 2)) - 0.5) * 24).astype(np.float32),  # up to +-12 px: samples clamp at every border
             ((rng.random((h, w, 2)) - 0.5) * 3).astype(np.float32),
             rng.integers(-12, 13, (h, w, 2)).astype(np.float32),  # exact integers: fx = fy = 0
             np.zeros((h, w, 2), np.float32)]
    for k, flow in enumerate(flows):
        got = fe.warp_coefficients(i1, i2, flow)
        want = W.coefficients_f32(i1, i2, flow)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (w, h, k, float(np.abs(got - want).max()))
    assert np.array_equal(fe.warp_coefficients(i1, i2, flows[3]), none)  # (a zero flow is the null flow)


@pytest.mark.parametrize("iterations", [1, 7])
@pytest.mark.parametrize("given_start", [False, True])
def test_horn_schunck_coef_equals_horn_schunck(nsc, iterations, given_start):
    w, h = 67, 45
    rng = np.random.default_rng(7)
    i1, i2 = rng.random((h, w, 4), np.float32), rng.random((h, w, 4), np.float32)
    start = ((rng.random((h, w, 2)) - 0.5) * 4).astype(np.float32) if given_start else None
    fe = nsc.FlowEstimator()
    coef = fe.warp_coefficients(i1, i2, None)
    for tiled in (0, 1, 2, 3):
        fe.set_tiled(tiled)
        got = fe.horn_schunck_coef(coef, start, iterations, 4e-4)
        want = fe.horn_schunck(i1, i2, start, iterations, 4e-4)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), tiled
    assert np.array_equal(got, W.jacobi_coef_f32(coef, start, iterations, 4e-4))


# ---- the estimator ----------------------------------------------------------------------------------------------------------------
def _composition(fe, a, b, warps):
    """blur / downsample / upsample / warp_coefficients / horn_schunck_coef, horn_schunck for the coarsest level."""
    def pyramid(frame):
        cur, out = fe.rgba8_to_f32(frame), []
        for level in range(P["levels"]):
            cur = fe.blur(cur)
            out.append(cur)
            if level + 1 < P["levels"]:
                cur = fe.downsample(cur)
        return out

    pa, pb = pyramid(a), pyramid(b)
    flow = fe.horn_schunck(pa[-1], pb[-1], None, P["coarse_iters"], P["lam"])
    for level in range(P["levels"] - 2, -1, -1):
        h, w = pa[level].shape[:2]
        flow = fe.upsample(flow, w, h, 2.0)
        for _ in range(warps):
            flow = fe.horn_schunck_coef(fe.warp_coefficients(pa[level], pb[level], flow), flow, P["refine_iters"], P["lam"])
    return flow


@pytest.mark.parametrize("size", [(67, 45), (200, 72)])
@pytest.mark.parametrize("warps", [1, 2])
def test_exact_estimate_equals_the_composition_of_the_primitives(nsc, size, warps):
    w, h = size
    a, b = _pair(size)
    want = _composition(nsc.FlowEstimator(), a, b, warps)
    d = float(np.abs(want - _witness(size, warps)).max())
    print(f"{size} warps {warps}: composition against the float64 witness {d:.3g} px")
    assert d <= W.F32_TOLERANCE
    for tiled in (0, 1, 2, 3):
        got = _estimator(nsc, warps, "exact", tiled).estimate(a, b, w, h)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tiled, float(np.abs(got - want).max()))


@pytest.mark.parametrize("size", [(67, 45), (200, 72)])
@pytest.mark.parametrize("warps", [1, 2])
@pytest.mark.parametrize("mode,tiled", [("exact", 1), ("fast", 1), ("fast", 3)])  # (fast, 3): the FAST kernels whatever the size
def test_estimate_against_the_float64_witness(nsc, size, warps, mode, tiled):
    w, h = size
    a, b = _pair(size)
    got = _estimator(nsc, warps, mode, tiled).estimate(a, b, w, h)
    d = float(np.abs(got - _witness(size, warps)).max())
    tol = W.F32_TOLERANCE + (FAST_CONTRACT if mode == "fast" else 0.0)
    print(f"{size} warps {warps} {mode} tiled {tiled}: {d:.3g} px from the float64 witness (tolerance {tol:.3g})")
    assert d <= tol
    # and the mode is on: the estimate is not the one without it
    assert float(np.abs(got - _witness(size, 0)).max()) > 0.5


# ---- device streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(67, 45), (192, 128)])
@pytest.mark.parametrize("mode,tiled", [("exact", 1), ("exact", 2), ("exact", 3), ("exact", 0), ("fast", 1), ("fast", 3)])
def test_stream_flows_equal_the_pair_entry_point(nsc, w, h, mode, tiled):
    import torch

    n = 4
    frames = _sequence(w, h, n)
    d = put(frames, "cuda:0")
    fb = w * h * 4
    exact = _estimator(nsc, 1, "exact", 1)
    want = []
    for k in range(n - 1):
        fl = guarded.empty((h, w, 2), dtype=torch.float32, device="cuda:0")
        exact.estimate_device(d.data_ptr() + k * fb, d.data_ptr() + (k + 1) * fb, w, h, fl.data_ptr(), _stream())
        want.append(fetch(fl))
    want = np.stack(want)
    assert float(np.abs(want).max()) > 1.5  # motion of more than a pixel
    flows = guarded.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda:0")
    _estimator(nsc, 1, mode, tiled).estimate_device_stream(d.data_ptr(), n, w, h, flows.data_ptr(), _stream())
    got = fetch(flows)
    assert np.array_equal(fetch(d), frames)  # the frames are inputs
    if mode == "exact":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), [float(np.abs(got[k] - want[k]).max()) for k in range(n - 1)]
    else:
        dist = float(np.abs(got - want).max())
        print(f"{w}x{h} fast tiled {tiled}: {dist:.3g} px from the exact flows")
        assert dist <= FAST_CONTRACT


@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("mode,tiled", [("exact", 1), ("fast", 3)])
def test_interpolate_multi_stream(nsc, ffmt, mode, tiled):
    import torch

    w, h, n = 192, 128, 4
    times = [0.25, 0.5, 0.75]
    frames = _sequence(w, h, n)
    frames[3, ..., :3] = frames[3, ::-1, ::-1, :3] // 4 + 180  # a cut in front of the last frame: another, brighter shot
    cuts = [1 if sc.is_cut(*sc.measures(frames[k], frames[k + 1]), w, h) else 0 for k in range(n - 1)]
    assert cuts == [0, 0, 1]
    d = put(frames, "cuda:0")
    fb = w * h * 4
    fdt = torch.float32 if ffmt == "f32" else torch.float16
    warp = nsc.WgpuFrameInterpolator()
    warp.set_mode("fma")
    warp.set_flow_format(ffmt)
    res = {}
    for scene_detect in (False, True):
        fe = _estimator(nsc, 1, mode, tiled)
        fe.set_scene_detect(scene_detect)
        mid = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
        flows = guarded.empty((n - 1, h, w, 2), dtype=fdt, device="cuda:0")
        fe.interpolate_multi_device_stream(d.data_ptr(), n, w, h, times, mid.data_ptr(), flows.data_ptr(), 0, _stream(), flow_format=ffmt)
        res[scene_detect] = (fetch(mid), fetch(flows))
    got_mid, got_flows = res[False]
    assert np.array_equal(res[True][1].view(np.uint8), got_flows.view(np.uint8))  # the flows do not depend on the detector
    # the frames: the multi-time warp in FMA mode on the flows the same call returned
    want = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
    d_flows = put(got_flows, "cuda:0")
    warp.interpolate_multi_device(d.data_ptr(), fb, d.data_ptr() + fb, fb, d_flows.data_ptr(), w, h, times, want.data_ptr(), 0, n - 1, _stream())
    assert np.array_equal(got_mid, fetch(want))
    # the flows: estimate_device_stream's, in f16 rounded to nearest even
    f32 = guarded.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda:0")
    _estimator(nsc, 1, mode, tiled).estimate_device_stream(d.data_ptr(), n, w, h, f32.data_ptr(), _stream())
    f32 = fetch(f32)
    assert float(np.abs(f32[:2]).max()) > 1.5
    if ffmt == "f32":
        assert np.array_equal(got_flows.view(np.uint32), f32.view(np.uint32))
    else:
        assert np.array_equal(got_flows.view(np.uint16), f32.astype(np.float16).view(np.uint16))
    # with the detector on the flagged pair's frames are repeats of the nearer frame, the others the same bytes
    on = res[True][0]
    assert np.array_equal(on[:2], got_mid[:2])
    assert np.array_equal(on[2, 0], frames[2]) and np.array_equal(on[2, 1], frames[3]) and np.array_equal(on[2, 2], frames[3])
    assert not np.array_equal(got_mid[2], on[2])


def test_warps_zero_after_warps_one_equals_a_fresh_handle(nsc):
    import torch

    w, h, n = 192, 128, 4
    frames = _sequence(w, h, n)
    d = put(frames, "cuda:0")
    for mode, tiled in (("exact", 1), ("fast", 3)):
        used, fresh = _estimator(nsc, 1, mode, tiled), _estimator(nsc, 0, mode, tiled)
        out = {}
        for name, fe in (("used", used), ("fresh", fresh)):
            if name == "used":  # one pair and one stream with the mode on, then off
                scratch = guarded.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda:0")
                assert fe.estimate(frames[0], frames[1], w, h).shape == (h, w, 2)
                fe.estimate_device_stream(d.data_ptr(), n, w, h, scratch.data_ptr(), _stream())
                fe.set_warps(0)
            assert fe.warps == 0
            flows = guarded.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda:0")
            fe.estimate_device_stream(d.data_ptr(), n, w, h, flows.data_ptr(), _stream())
            mid = guarded.empty((n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
            half = guarded.empty((n - 1, h, w, 2), dtype=torch.float16, device="cuda:0")
            fe.interpolate_device_stream(d.data_ptr(), n, w, h, 0.5, mid.data_ptr(), half.data_ptr(), _stream(), "f16")
            torch.cuda.synchronize()  # (the host entry point runs on the handle's own stream, in the same workspace)
            out[name] = (fe.estimate(frames[0], frames[1], w, h), fetch(flows), fetch(mid), fetch(half))
        for x, y in zip(out["used"], out["fresh"]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), mode
        if mode == "exact":  # and warps = 0 is the estimator the oracle restates
            import oracle

            assert np.array_equal(out["fresh"][0], oracle.flow_estimate(frames[0], frames[1], P["levels"], P["coarse_iters"],
                                                                        P["refine_iters"], P["lam"]))


# ---- what it is for ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in W.ROWS if (r[0], r[1]) == (192, 128)], ids=lambda r: f"pan{r[2]}mv{r[3]}".replace(" ", ""))
def test_in_between_frame_is_nearer_the_true_one(nsc, row):
    w, h = row[:2]
    a, b, true_mid = W.scene(row)
    psnr = {}
    for warps in (0, 1):
        it = nsc.PyFrameInterpolator("optical_flow", flow_warps=warps)
        it.initialize(w, h)
        got = np.frombuffer(it.interpolate(a.tobytes(), b.tobytes(), 0.5), np.uint8).reshape(h, w, 4)
        psnr[warps] = scenes.psnr_rgb(got, true_mid)
    print(f"{row}: flow_warps 0 {psnr[0]:.2f} dB, flow_warps 1 {psnr[1]:.2f} dB")
    assert psnr[1] >= psnr[0] + 2.0


def test_both_clis_write_the_same_png(nsc, tmp_path):
    from nu_scaler_amd.imagefile import read_png, write_png

    row = W.ROWS[0]
    w, h = row[:2]
    a, b, _ = W.scene(row)
    write_png(str(tmp_path / "a.png"), w, h, a.tobytes())
    write_png(str(tmp_path / "b.png"), w, h, b.tobytes())
    native = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    assert os.path.exists(native)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for name, cmd in (("native", [native]), ("py", [sys.executable, "-m", "nu_scaler_amd.cli"])):
        r = subprocess.run([*cmd, "interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png"), str(tmp_path / f"{name}.png"), "--flow",
                            "--flow-warps", "1"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr
    assert open(tmp_path / "native.png", "rb").read() == open(tmp_path / "py.png", "rb").read()
    it = nsc.PyFrameInterpolator("optical_flow", flow_warps=1)
    it.initialize(w, h)
    assert read_png(str(tmp_path / "py.png"))[2] == it.interpolate(a.tobytes(), b.tobytes(), 0.5)
    plain = nsc.PyFrameInterpolator("optical_flow")
    plain.initialize(w, h)
    assert read_png(str(tmp_path / "py.png"))[2] != plain.interpolate(a.tobytes(), b.tobytes(), 0.5)


def test_step_motion_takes_the_setting(nsc, oracle_mod):
    """FramePipeline.step_motion(flow_warps=1): the flows of estimate_device_stream with warps = 1, the in-between frames warped with
    them; fused_warp (one entry point, Rg16Float hand-off in FAST) likewise; flow_warps=0 on the same pipeline is the step without."""
    import torch

    w, h, n = 192, 128, 3
    frames = _sequence(w, h, n + 1)
    dev = torch.device("cuda:0")
    d = put(frames, "cuda:0")
    s = _stream()
    pipe = nsc.FramePipeline(w, h, 2, "lanczos3", 0.5, lanczos_mode="exact")
    want = {}
    for warps in (0, 1):
        fl = guarded.empty((n, h, w, 2), dtype=torch.float32, device=dev)
        _estimator(nsc, warps).estimate_device_stream(d.data_ptr(), n + 1, w, h, fl.data_ptr(), s)
        want[warps] = fetch(fl)
    assert float(np.abs(want[1] - want[0]).max()) > 0.5
    for warps in (1, 0, 1):
        mid, up_real, up_mid = guarded.like(pipe.alloc(n, dev))
        flows = guarded.empty((n, h, w, 2), dtype=torch.float32, device=dev)
        pipe.step_motion(d, flows, mid, up_real, up_mid, s, flow_warps=warps)
        assert np.array_equal(fetch(flows).view(np.uint32), want[warps].view(np.uint32)), warps
        for k in range(n):
            want_mid = oracle_mod.warp_blend(frames[k], frames[k + 1], want[warps][k], 0.5)
            assert np.array_equal(fetch(mid[k]), want_mid), (warps, k)
            assert np.array_equal(fetch(up_mid[k]), oracle_mod.lanczos3(want_mid, 2 * w, 2 * h)), (warps, k)
    # one entry point for estimator and warp, FAST, the flows as Rg16Float between them and not stored
    fast = nsc.FramePipeline(w, h, 2, "lanczos3", 0.5)
    fma = nsc.WgpuFrameInterpolator()
    fma.set_mode("fma")
    fma.set_flow_format("f16")
    half = guarded.empty((n, h, w, 2), dtype=torch.float16, device=dev)
    fe = _estimator(nsc, 1, "fast", 1)
    scratch = guarded.empty((n, h, w, 4), dtype=torch.uint8, device=dev)
    fe.interpolate_device_stream(d.data_ptr(), n + 1, w, h, 0.5, scratch.data_ptr(), half.data_ptr(), s, "f16")
    want_mid = guarded.empty((n, h, w, 4), dtype=torch.uint8, device=dev)
    fb = w * h * 4
    fma.interpolate_device(d.data_ptr(), fb, d.data_ptr() + fb, fb, half.data_ptr(), w, h, 0.5, want_mid.data_ptr(), n, s)
    mid, up_real, up_mid = guarded.like(fast.alloc(n, dev))
    fast.step_motion(d, None, mid, up_real, up_mid, s, flow_mode="fast", fused_warp=True, flow_warps=1)
    assert np.array_equal(fetch(mid), fetch(want_mid)) and np.array_equal(fetch(scratch), fetch(want_mid))
    with pytest.raises(ValueError, match="warps"):
        fast.step_motion(d, None, mid, up_real, up_mid, s, flow_mode="fast", fused_warp=True, flow_warps=5)
