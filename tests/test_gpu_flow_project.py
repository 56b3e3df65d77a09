"""The projection rounds of the dense-flow warp on the GPU (nus_interp_set_flow_project, nus_flow_set_project, nus_flow_project):
the projection alone against its float32 restatement as values (tests/_flow_project.py), EXACT frames byte for byte against the
oracle's warp + blend with the projected vectors, FMA frames under the warp contract with those vectors as the flow, the
interpolating entry points of the estimator against estimate followed by the projecting warp, rounds = 0 after rounds = 3
against fresh handles, and what the mode is for: the in-between frame on scenes with a known true mid-frame.  Every device
output comes from conftest.guarded."""
import functools

import numpy as np
import pytest

import _bm_bidir as scenes
import _flow_project as PJ
import _flow_warp64 as W
import oracle
from _warp64 import warp_contract
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

P = W.PARAMS
TABLE = (P["levels"], P["coarse_iters"], P["refine_iters"])
ROUNDS = (1, 2, 3, 4)
FMA_POSITION_ULPS = 0.5  # the FMA-mode warp's sample position is one fused multiply-add (tests/test_gpu_warp_fma_contract.py)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _t32(t):
    return float(np.float32(t))


# ---- the CPU inputs and references: once per module run, read-only -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flows(w, h):
    """(3, h, w, 2) float32: smooth random vectors of +-12 px, a motion boundary (a quadrant that moves another way, sub-pixel parts
    included), and vectors that leave the frame -- three different flows for three pairs."""
    rng = np.random.default_rng(7001 + 31 * w + h)
    coarse = (rng.random((h // 8 + 2, w // 8 + 2, 2)) - 0.5) * 24
    yy, xx = np.mgrid[0:h, 0:w]
    y0, x0, fy, fx = yy // 8, xx // 8, (yy % 8 / 8.0)[..., None], (xx % 8 / 8.0)[..., None]
    smooth = ((coarse[y0, x0] * (1 - fx) + coarse[y0, x0 + 1] * fx) * (1 - fy)
              + (coarse[y0 + 1, x0] * (1 - fx) + coarse[y0 + 1, x0 + 1] * fx) * fy).astype(np.float32)
    step = np.full((h, w, 2), (-3.25, 1.5), np.float32)
    step[h // 2:, w // 2:] = (7.5, -2.75)
    outside = ((rng.random((h, w, 2)) - 0.5) * 6).astype(np.float32)
    outside[::3, 1::2] += (2.0 * w + 0.5, -1.5 * h - 0.25)
    outside[1::3, ::2] -= (1.25 * w, -3.0 * h)
    out = np.stack([smooth, step, outside])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    f = np.random.default_rng(7101 + 31 * w + h).integers(0, 256, (4, h, w, 4), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _projected(w, h, ffmt, t, rounds):
    """The restatement's vectors for the three flows of a size, from the flow as the warp reads it (f16: rounded to half, widened)."""
    flows = _flows(w, h)
    if ffmt == "f16":
        flows = flows.astype(np.float16).astype(np.float32)
    out = np.stack([PJ.project_f32(f, t, rounds) for f in flows])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want_exact(w, h, ffmt, t, rounds, bgra=False):
    frames = _frames(w, h)
    if bgra:
        frames = frames[..., [2, 1, 0, 3]]
    g = _projected(w, h, ffmt, t, rounds)
    out = np.stack([oracle.warp_blend(np.ascontiguousarray(frames[i]), np.ascontiguousarray(frames[i + 1]), g[i], t) for i in range(3)])
    out.setflags(write=False)
    return out


def _assert_values(got, want, tag):
    assert got.dtype == np.float32 and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        diff = got != want
        first = tuple(int(v) for v in np.argwhere(diff)[0])
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(got.astype(np.float64) - want)))
        raise AssertionError(f"{tag}: {int(diff.sum())} of {diff.size} floats differ, max |difference| {worst:.3g} px, first differing cell "
                             f"(y, x, component) {first}: got {float(got[first])!r}, want {float(want[first])!r}")


def _assert_bytes(got, want, tag):
    assert got.dtype == np.uint8 and got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        diff = got != want
        first = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{tag}: {int(diff.sum())} of {diff.size} bytes differ, largest difference "
                             f"{int(np.abs(got.astype(int) - want).max())}, first at {first}: got {int(got[first])}, want {int(want[first])}")


def _interp(nsc, rounds, mode="exact", ffmt="f32", fmt="rgba"):
    it = nsc.WgpuFrameInterpolator()
    it.set_mode(mode)
    it.set_flow_format(ffmt)
    it.set_input_format(fmt)
    it.set_flow_project(rounds)
    assert it.flow_project == rounds
    return it


def _device_flows(w, h, ffmt):
    flows = _flows(w, h)
    return put(np.ascontiguousarray(flows if ffmt == "f32" else flows.astype(np.float16)))


def _single(it, d_frames, d_flow, w, h, t, n=3):
    import torch

    fb = w * h * 4
    out = guarded.empty((n, h, w, 4), dtype=torch.uint8, device="cuda:0")
    it.interpolate_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_flow.data_ptr(), w, h, t, out.data_ptr(), n, _stream())
    return fetch(out)


def _multi(it, d_frames, d_flow, w, h, times, n=3, gap=0):
    """-> (n, len(times), h, w, 4); gap: that many frames of room behind every pair's frames (out_pair_stride), checked untouched."""
    import torch

    fb = w * h * 4
    k = len(times)
    out = guarded.full((n, k + gap, h, w, 4), 0xA5, dtype=torch.uint8, device="cuda:0")
    it.interpolate_multi_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_flow.data_ptr(), w, h, times, out.data_ptr(),
                                (k + gap) * fb if gap else 0, n, _stream())
    got = fetch(out)
    assert (got[:, k:] == 0xA5).all()  # nothing stored into the gap
    return got[:, :k]


# ---- the projection alone ---------------------------------------------------------------------------------------------------------------
# 1 x 1, 2 x 1, 1 x 2: the plain form; 5 x 3: the smallest corner form; odd and even widths; a last row block that is not full
@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 2), (5, 3), (67, 45), (130, 70), (66, 9)])
def test_projection_equals_the_float32_restatement(nsc, w, h):
    fe = nsc.FlowEstimator()
    moved = 0
    for name, flow in zip(("smooth", "step", "outside"), _flows(w, h)):
        for t in (0.0, 0.25, 0.5, 1.0):
            for rounds in ROUNDS:
                got = fe.project_flow(flow, t, rounds)
                want = PJ.project_f32(flow, t, rounds)
                _assert_values(got, want, (w, h, name, t, rounds))
                moved += int((want != flow).any())
            if t == 0.0:
                assert np.array_equal(got, flow), (w, h, name)  # t = 0: g = f(p)
        assert np.array_equal(fe.project_flow(flow, 0.5, 0), flow), (w, h, name)  # rounds 0 copies
    assert moved > 0 or (w, h) == (1, 1)  # (the rounds do something on these flows)
    assert fe.project == 0  # the primitive is not the setting


# ---- EXACT: the frame is the oracle's warp + blend with the projected vectors, byte for byte ---------------------------------------------
@pytest.mark.parametrize("w,h", [(67, 45), (130, 70)])
def test_exact_host_entry_point(nsc, w, h):
    frames, flows = _frames(w, h), _flows(w, h)
    for rounds, t in ((1, 0.5), (2, 0.25), (3, 0.5), (4, 1.0)):
        it = _interp(nsc, rounds)
        want = _want_exact(w, h, "f32", t, rounds)
        for i in range(3):
            got = np.frombuffer(it.interpolate_py(frames[i].tobytes(), frames[i + 1].tobytes(), w, h, time_t=t, flow=flows[i]), np.uint8)
            _assert_bytes(got.reshape(h, w, 4), want[i], ("interpolate", w, h, rounds, t, i))
    # the multi-time host entry point projects per time
    times = [_t32(0.25), 0.5, _t32(0.7)]
    it = _interp(nsc, 3)
    for i in range(3):
        got = it.interpolate_multi_py(frames[i].tobytes(), frames[i + 1].tobytes(), w, h, times=times, flow=flows[i])
        for k, t in enumerate(times):
            _assert_bytes(np.frombuffer(got[k], np.uint8).reshape(h, w, 4), _want_exact(w, h, "f32", t, 3)[i], ("interpolate_multi", w, h, t, i))
    # no flow: the unchanged zero-flow blend
    got = np.frombuffer(it.interpolate_py(frames[0].tobytes(), frames[1].tobytes(), w, h, time_t=0.5), np.uint8).reshape(h, w, 4)
    _assert_bytes(got, oracle.warp_blend(frames[0], frames[1], None, 0.5), ("zero flow", w, h))


# three pairs with three different flows: a gather into a neighbouring pair's plane shows up as wrong bytes
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", [(67, 45), (130, 70), (66, 9), (2, 1), (1, 2)])
def test_exact_device_entry_points(nsc, w, h, ffmt):
    d_frames, d_flow = put(np.ascontiguousarray(_frames(w, h))), _device_flows(w, h, ffmt)
    times3 = [_t32(0.25), 0.5, _t32(0.7)]
    times7 = [_t32(k / 8) for k in range(1, 8)]
    for rounds in ROUNDS:
        it = _interp(nsc, rounds, "exact", ffmt)
        for t in (0.5, _t32(0.3)) if rounds in (1, 3) else (0.5,):
            _assert_bytes(_single(it, d_frames, d_flow, w, h, t), _want_exact(w, h, ffmt, t, rounds), ("interpolate_device", w, h, ffmt, rounds, t))
        for times, gap in ((times3, 0), (times3, 1), (times7, 0)) if rounds in (2, 3) else ((times3, 0),):
            got = _multi(it, d_frames, d_flow, w, h, times, gap=gap)
            for k, t in enumerate(times):
                _assert_bytes(got[:, k], _want_exact(w, h, ffmt, t, rounds), ("interpolate_multi_device", w, h, ffmt, rounds, len(times), gap, t))
    # the setting is on: other bytes than the plain warp's
    if w > 2:
        assert not np.array_equal(_want_exact(w, h, ffmt, 0.5, 2), _single(_interp(nsc, 0, "exact", ffmt), d_frames, d_flow, w, h, 0.5))


@pytest.mark.parametrize("w,h", [(67, 45), (130, 70)])
def test_exact_bgra_input(nsc, w, h):
    d_frames, d_flow = put(np.ascontiguousarray(_frames(w, h))), _device_flows(w, h, "f32")
    it = _interp(nsc, 2, "exact", "f32", "bgra")
    _assert_bytes(_single(it, d_frames, d_flow, w, h, 0.5), _want_exact(w, h, "f32", 0.5, 2, True), ("bgra interpolate_device", w, h))
    times = [_t32(0.25), 0.5, _t32(0.7)]
    got = _multi(it, d_frames, d_flow, w, h, times)
    for k, t in enumerate(times):
        _assert_bytes(got[:, k], _want_exact(w, h, "f32", t, 2, True), ("bgra interpolate_multi_device", w, h, t))


# ---- FMA: the warp contract with the projected vectors as the flow -------------------------------------------------------------------------
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", [(67, 45), (130, 70)])
def test_fma_frames_meet_the_warp_contract(nsc, w, h, ffmt):
    frames = _frames(w, h)
    d_frames, d_flow = put(np.ascontiguousarray(frames)), _device_flows(w, h, ffmt)
    times = [_t32(0.25), 0.5, _t32(0.7)]
    for rounds in (1, 2, 3):
        it = _interp(nsc, rounds, "fma", ffmt)
        single = _single(it, d_frames, d_flow, w, h, 0.5)
        multi = _multi(it, d_frames, d_flow, w, h, times)
        assert np.array_equal(multi[:, 1], single)
        for k, t in enumerate(times):  # (per time: the vectors depend on it)
            st = warp_contract(multi[:, k], frames[:3], frames[1:], _projected(w, h, ffmt, t, rounds), t, FMA_POSITION_ULPS,
                               ("fma", w, h, ffmt, rounds, t))
            print(f"FMA project {w}x{h} {ffmt} rounds {rounds} t {t}: samples {st['samples']}, decided {st['decided'] / st['samples']:.4f}, "
                  f"differ from all-floor {st['differ_from_floor'] / st['samples']:.2e}")
            assert st["decided"] / st["samples"] >= 0.9


# ---- the estimator's interpolating entry points ---------------------------------------------------------------------------------------------
def _sequence(w, h, n, pan=(1, 0), mv=(2, 1), sq=24, seed=3):
    """n frames of _bm_bidir.scene's kind: the background pans by `pan` per frame, the square moves by `mv` per frame."""
    rng = np.random.default_rng(seed)
    m = 16
    bg = scenes.smooth_noise(rng, h + 2 * m, w + 2 * m)
    fg = scenes.smooth_noise(rng, sq, sq, 1)
    out = []
    for k in range(n):
        im = bg[m + pan[1] * k:m + pan[1] * k + h, m + pan[0] * k:m + pan[0] * k + w].copy()
        x0, y0 = 10 + mv[0] * k, 8 + mv[1] * k
        im[y0:y0 + sq, x0:x0 + sq] = fg
        out.append(np.dstack([im, np.full((h, w), 255, np.uint8)]))
    return np.stack(out)


def _estimator(nsc, mode, tiled, project=0, warps=1, median=5):
    fe = nsc.FlowEstimator(TABLE[0], TABLE[1], TABLE[2], P["lam"], warps=warps, median=median, project=project)
    fe.set_mode(mode)
    fe.set_tiled(tiled)
    assert fe.project == project
    return fe


@pytest.mark.parametrize("w,h", [(67, 45), (192, 128)])
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("mode,tiled", [("exact", 1), ("fast", 3)])
@pytest.mark.parametrize("chunk", [None, "2"])
def test_interpolating_entry_points_equal_estimate_then_projecting_warp(nsc, monkeypatch, w, h, ffmt, mode, tiled, chunk):
    import torch

    if chunk is None:
        monkeypatch.delenv("NUS_FLOW_MAX_CHUNK_PAIRS", raising=False)
    else:
        monkeypatch.setenv("NUS_FLOW_MAX_CHUNK_PAIRS", chunk)  # 4 pairs in chunks of 2 + 2
    n, rounds = 5, 2
    times = [0.25, 0.5, 0.75]
    frames = _sequence(w, h, n)
    d = put(frames, "cuda:0")
    fb = w * h * 4
    fdt = torch.float32 if ffmt == "f32" else torch.float16
    s = _stream()
    f32 = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    _estimator(nsc, mode, tiled, rounds).estimate_device_stream(d.data_ptr(), n, w, h, f32.data_ptr(), s)  # (project: not its business)
    f32 = fetch(f32)
    plain = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    _estimator(nsc, mode, tiled, 0).estimate_device_stream(d.data_ptr(), n, w, h, plain.data_ptr(), s)
    assert np.array_equal(f32.view(np.uint32), fetch(plain).view(np.uint32))  # the flows are unchanged by the setting
    assert float(np.abs(f32).max()) > 1.5
    want_flows = f32 if ffmt == "f32" else f32.astype(np.float16)
    d_flows = put(want_flows, "cuda:0")
    warp = _interp(nsc, rounds, "fma", ffmt)
    want_multi = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
    warp.interpolate_multi_device(d.data_ptr(), fb, d.data_ptr() + fb, fb, d_flows.data_ptr(), w, h, times, want_multi.data_ptr(), 0, n - 1, s)
    want_multi = fetch(want_multi)
    warp.set_flow_project(0)
    unprojected = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
    warp.interpolate_multi_device(d.data_ptr(), fb, d.data_ptr() + fb, fb, d_flows.data_ptr(), w, h, times, unprojected.data_ptr(), 0, n - 1, s)
    assert not np.array_equal(want_multi, fetch(unprojected))  # the setting is on
    for with_flows in (True, False):
        fe = _estimator(nsc, mode, tiled, rounds)
        flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=fdt, device="cuda:0")
        mid = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
        fe.interpolate_multi_device_stream(d.data_ptr(), n, w, h, times, mid.data_ptr(), flows.data_ptr() if with_flows else 0, 0, s, flow_format=ffmt)
        _assert_bytes(fetch(mid), want_multi, (w, h, ffmt, mode, tiled, chunk, with_flows, "multi"))
        if with_flows:
            assert np.array_equal(fetch(flows).view(np.uint8), want_flows.view(np.uint8)), (ffmt, mode, tiled, "multi flows")
        else:
            assert np.isnan(fetch(flows).astype(np.float32)).all()  # nothing was stored there
        flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=fdt, device="cuda:0")
        one = guarded.empty((n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
        fe.interpolate_device_stream(d.data_ptr(), n, w, h, 0.5, one.data_ptr(), flows.data_ptr() if with_flows else 0, s, ffmt)
        _assert_bytes(fetch(one), want_multi[:, 1], (w, h, ffmt, mode, tiled, chunk, with_flows, "single"))
        if with_flows:
            assert np.array_equal(fetch(flows).view(np.uint8), want_flows.view(np.uint8)), (ffmt, mode, tiled, "single flows")
    assert np.array_equal(fetch(d), frames)  # the frames are inputs


# ---- off means off ---------------------------------------------------------------------------------------------------------------------------
def test_rounds_zero_after_rounds_three_equals_fresh_handles(nsc):
    import torch

    w, h, n = 130, 70, 4
    frames = _sequence(w, h, n)
    d = put(frames, "cuda:0")
    s = _stream()
    times = [0.25, 0.5, 0.75]
    # the estimator's handle: bytes and workspace
    for mode, tiled in (("exact", 1), ("fast", 3)):
        out, workspace = {}, {}
        for name in ("used", "fresh"):
            fe = _estimator(nsc, mode, tiled, 3 if name == "used" else 0)
            if name == "used":  # the same two calls with the rounds on, then off
                scratch = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
                scratch_flows = guarded.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda:0")
                fe.interpolate_multi_device_stream(d.data_ptr(), n, w, h, times, scratch.data_ptr(), scratch_flows.data_ptr(), 0, s)
                fe.interpolate_device_stream(d.data_ptr(), n, w, h, 0.5, scratch.data_ptr(), scratch_flows.data_ptr(), s, "f16")
                torch.cuda.synchronize()
                fe.set_project(0)
            assert fe.project == 0
            flows = guarded.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda:0")
            mid = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
            fe.interpolate_multi_device_stream(d.data_ptr(), n, w, h, times, mid.data_ptr(), flows.data_ptr(), 0, s)
            half = guarded.empty((n - 1, h, w, 2), dtype=torch.float16, device="cuda:0")
            one = guarded.empty((n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
            fe.interpolate_device_stream(d.data_ptr(), n, w, h, 0.5, one.data_ptr(), half.data_ptr(), s, "f16")
            torch.cuda.synchronize()
            out[name] = (fetch(flows), fetch(mid), fetch(half), fetch(one))
            workspace[name] = fe.workspace_bytes
        for x, y in zip(out["used"], out["fresh"]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), mode
        assert workspace["used"] == workspace["fresh"] > 0, (mode, workspace)  # the rounds reserved nothing
    # the interpolator's handle: bytes, and the oracle's with the plain flow
    flows3 = _flows(w, h)
    d_frames, d_flow = put(np.ascontiguousarray(_frames(w, h))), _device_flows(w, h, "f32")
    for mode in ("exact", "fma"):
        used, fresh = _interp(nsc, 3, mode), _interp(nsc, 0, mode)
        assert not np.array_equal(_single(used, d_frames, d_flow, w, h, 0.5), _single(fresh, d_frames, d_flow, w, h, 0.5))
        _multi(used, d_frames, d_flow, w, h, times)
        used.set_flow_project(0)
        assert used.flow_project == 0
        got = _single(used, d_frames, d_flow, w, h, 0.5)
        assert np.array_equal(got, _single(fresh, d_frames, d_flow, w, h, 0.5)), mode
        assert np.array_equal(_multi(used, d_frames, d_flow, w, h, times), _multi(fresh, d_frames, d_flow, w, h, times)), mode
        if mode == "exact":
            fr = _frames(w, h)
            for i in range(3):
                _assert_bytes(got[i], oracle.warp_blend(fr[i], fr[i + 1], flows3[i], 0.5), ("rounds 0", i))


# ---- what it is for ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [W.ROWS[1], W.ROWS[5]], ids=lambda r: f"pan{r[2]}mv{r[3]}".replace(" ", ""))
def test_in_between_frame_is_nearer_the_true_one(nsc, row):
    w, h = row[:2]
    a, b, true_mid = W.scene(row)
    psnr = {}
    for rounds in (0, 3):
        it = nsc.PyFrameInterpolator("optical_flow", flow_warps=2, flow_median=5, flow_project=rounds)
        it.initialize(w, h)
        got = np.frombuffer(it.interpolate(a.tobytes(), b.tobytes(), 0.5), np.uint8).reshape(h, w, 4)
        psnr[rounds] = scenes.psnr_rgb(got, true_mid)
    print(f"{row}: flow_warps 2, flow_median 5: flow_project 0 {psnr[0]:.2f} dB, flow_project 3 {psnr[3]:.2f} dB")
    assert psnr[3] > psnr[0]


def test_step_motion_fused_and_unfused_agree(nsc):
    import torch

    w, h, n = 192, 128, 3
    frames = _sequence(w, h, n + 1)
    dev = torch.device("cuda:0")
    d = put(frames, "cuda:0")
    s = _stream()
    pipe = nsc.FramePipeline(w, h, 2, "lanczos3", 0.5, lanczos_mode="exact")
    pipe.interp.set_mode("fma")  # the fused route's warp is the FMA-mode one
    mids = {}
    for rounds, fused in ((2, False), (2, True), (0, False), (0, True), (2, True)):
        mid, up_real, up_mid = guarded.like(pipe.alloc(n, dev))
        flows = guarded.empty((n, h, w, 2), dtype=torch.float32, device=dev)
        pipe.step_motion(d, flows, mid, up_real, up_mid, s, flow_warps=1, flow_median=5, fused_warp=fused, flow_format="f32",
                         flow_project=rounds)
        assert (pipe._flow.project, pipe.interp.flow_project) == (rounds, rounds)
        got = fetch(mid)
        if (rounds, fused) in mids:
            assert np.array_equal(got, mids[rounds, fused])  # back on: the same bytes again
        mids[rounds, fused] = got
        if fused:
            _assert_bytes(got, mids[rounds, False], ("step_motion", rounds))
            g = np.stack([PJ.project_f32(f, 0.5, rounds) for f in fetch(flows)])
            warp_contract(got, frames[:-1], frames[1:], g, 0.5, FMA_POSITION_ULPS, ("step_motion", rounds))
    assert not np.array_equal(mids[2, True], mids[0, True])
    with pytest.raises(ValueError, match="projection rounds"):
        pipe.step_motion(d, flows, mid, up_real, up_mid, s, flow_project=5)
