"""nus_flow_set_median on the GPU: the kernel alone against the numpy median (tests/_flow_median.py), the EXACT estimator against
its float32 restatement as values, FAST within the header's bound, every entry point against the pair entry point and the warp,
median = 0 after median = 5 against a fresh handle, and what the mode is for: the in-between frame on scenes with a known true
mid-frame.  Flows through the median are compared as values (np.array_equal): a selection network and a sort may return either of
-0 and +0.  Every device output comes from conftest.guarded."""
import functools

import numpy as np
import pytest

import _bm_bidir as scenes
import _flow_median as M
import _flow_warp64 as W
import oracle
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

P = W.PARAMS  # levels 3, 50 + 10 steps, lambda 4e-4: the table's settings (and FlowEstimator's defaults)
TABLE = (P["levels"], P["coarse_iters"], P["refine_iters"])
FAST_CONTRACT = 1e-3  # px, nus_flow_set_mode(NUS_FLOW_FAST)
FAST_CONDITIONING = 4.0  # ... or this many times the exact f32 result's distance from the float64 witness, with warps (the header)
TILE = (64, 16)  # k_flow_median's tile


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _estimator(nsc, warps=0, median=0, mode="exact", tiled=1, params=TABLE):
    fe = nsc.FlowEstimator(params[0], params[1], params[2], P["lam"], warps=warps, median=median)
    fe.set_mode(mode)
    fe.set_tiled(tiled)
    assert (fe.warps, fe.median_size) == (warps, median)
    return fe


# ---- the CPU references: once per module run, read-only --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(size):
    """(a, b) RGBA8: 67 x 45 is the top-left crop of the table's first scene, 200 x 72 its fourth scene; other sizes: the lattice's."""
    if size == (67, 45):
        a, b, _ = W.scene(W.ROWS[0])
        out = np.ascontiguousarray(a[:45, :67]), np.ascontiguousarray(b[:45, :67])
    elif size == (200, 72):
        out = tuple(np.ascontiguousarray(f) for f in W.scene(W.ROWS[3])[:2])
    else:
        out = tuple(W.lattice_frames(*size))
    for f in out:
        f.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _f32(size, params, warps, median):
    a, b = _pair(size)
    out = M.estimate_f32(oracle, a, b, params[0], params[1], params[2], P["lam"], warps=warps, median=median)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _f32_from_f64(size, params, warps, median):
    a, b = _pair(size)
    f64 = M.estimate(a, b, params[0], params[1], params[2], P["lam"], warps=warps, median=median)
    return float(np.abs(_f32(size, params, warps, median) - f64).max())


def _assert_values(got, want, tag):
    assert got.dtype == np.float32 and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        diff = got != want
        first = tuple(int(v) for v in np.argwhere(diff)[0])
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(got.astype(np.float64) - want)))
        raise AssertionError(f"{tag}: {int(diff.sum())} of {diff.size} floats differ, max |difference| {worst:.3g} px, first differing cell "
                             f"(.., y, x, component) {first}: got {float(got[first])!r}, want {float(want[first])!r}")


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


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------------
# a level smaller than the window, one narrower than the halo, tile edges crossed once and twice, one cell more than a tile each way
@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 2), (5, 3), (67, 45), (130, 70), (TILE[0] + 1, TILE[1] + 1)])
def test_median_kernel_equals_the_numpy_median(nsc, w, h):
    rng = np.random.default_rng(100 * w + h)
    fe = nsc.FlowEstimator()
    random = ((rng.random((h, w, 2)) - 0.5) * 24).astype(np.float32)  # +-12 px
    step = np.full((h, w, 2), (-3.25, 1.5), np.float32)  # two constant regions: a quadrant with a corner at (cx, cy)
    cx, cy = w // 2, h // 2
    step[cy:, cx:] = (7.5, -2.75)
    const = np.full((h, w, 2), (1.75, -0.5), np.float32)
    outliers = const.copy()
    outliers[3::7, 3::7] = (40.0, -40.0)  # 2 % of the cells, no two in one window
    yy, xx = np.mgrid[0:h, 0:w]
    for size in M.SIZES:
        r = size // 2
        for name, flow in (("random", random), ("step", step), ("outliers", outliers), ("all-equal", const)):
            got = fe.median(flow, size)
            _assert_values(got, M.median_filter(flow, size), (w, h, size, name))
        away = np.maximum(np.abs(xx - cx + 0.5), np.abs(yy - cy + 0.5)) > r + 0.5  # (further than the window's reach from the corner)
        assert np.array_equal(fe.median(step, size)[away], step[away]), (w, h, size)
        assert np.array_equal(fe.median(outliers, size), const), (w, h, size)
        assert np.array_equal(fe.median(const, size), const), (w, h, size)
        assert np.array_equal(fe.median(random, size)[..., 0], M.median_filter(random, size)[..., 0])  # (u and v separately)
    assert fe.median_size == 0  # the primitive is not the setting


# ---- EXACT: the estimator is the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(67, 45), (200, 72)])
@pytest.mark.parametrize("warps", [0, 1, 2])
@pytest.mark.parametrize("median", M.SIZES)
def test_exact_estimate_equals_the_float32_restatement(nsc, size, warps, median):
    w, h = size
    a, b = _pair(size)
    want = _f32(size, TABLE, warps, median)
    for tiled in (0, 1, 2, 3):
        got = _estimator(nsc, warps, median, "exact", tiled).estimate(a, b, w, h)
        _assert_values(got, want, (size, f"warps {warps}", f"median {median}", f"set_tiled({tiled})"))
    assert float(np.abs(want - _f32(size, TABLE, warps, 0)).max()) > 0.05  # the setting is on: another estimate


# 4 levels and odd sizes (130 x 71 -> 17 x 9), levels smaller than the window (5 x 3 -> 3 x 2 -> 2 x 1), and the runs of zero steps
@pytest.mark.parametrize("case", [c for c in W.LATTICE if c[:2] in ((130, 71), (5, 3)) or (c[:2] == (173, 70))], ids=W.lattice_id)
def test_exact_estimate_on_lattice_cases(nsc, case):
    size, params = case[:2], case[2:]
    w, h = size
    a, b = _pair(size)
    for warps in (0, 2):
        for median in M.SIZES:
            want = _f32(size, params, warps, median)
            for tiled in (0, 1, 2, 3):
                got = _estimator(nsc, warps, median, "exact", tiled, params).estimate(a, b, w, h)
                _assert_values(got, want, (W.lattice_id(case), f"warps {warps}", f"median {median}", f"set_tiled({tiled})"))
    if params[2] == 0:  # no refining steps: no run, no filter, on any finer level -- the filtered coarsest flow, upsampled twice
        coarse_only = _f32(size, params, 0, 5)
        assert np.array_equal(coarse_only, _f32(size, params, 2, 5))
        assert not np.array_equal(coarse_only, _f32(size, params, 0, 0))
    if params[1] == 0:  # no coarse steps: the finer levels start from the zero flow, unfiltered (a median of zeros is zero either way)
        assert float(np.abs(_f32(size, params, 2, 5)).max()) > 0.5


# ---- FAST: within the header's bound of the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(67, 45), (200, 72)])
@pytest.mark.parametrize("warps", [0, 1, 2])
@pytest.mark.parametrize("median", M.SIZES)
def test_fast_estimate_is_within_the_contract(nsc, size, warps, median):
    """max(1e-3 px, 4 x the float32 restatement's distance from the float64 witness on the same pair and settings): the rule the
    header states for warps."""
    w, h = size
    a, b = _pair(size)
    want = _f32(size, TABLE, warps, median)
    d64 = _f32_from_f64(size, TABLE, warps, median)
    bound = max(FAST_CONTRACT, FAST_CONDITIONING * d64)
    for tiled in (1, 2, 3):
        got = _estimator(nsc, warps, median, "fast", tiled).estimate(a, b, w, h)
        assert np.isfinite(got).all()
        d = float(np.abs(got.astype(np.float64) - want).max())
        print(f"FAST median | {w}x{h} | warps {warps} | median {median} | set_tiled({tiled}) | {d:.2e} px | exact f32 from float64 {d64:.2e} px | "
              f"bound {bound:.2e}")
        assert d <= bound, (size, warps, median, tiled, d, d64)


# ---- entry points ------------------------------------------------------------------------------------------------------------------
def _pair_flows(nsc, d, n, w, h, warps, median):
    """estimate_device, pair by pair, EXACT."""
    import torch

    fe = _estimator(nsc, warps, median, "exact", 1)
    fb = w * h * 4
    out = []
    for k in range(n - 1):
        fl = guarded.full((h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
        fe.estimate_device(d.data_ptr() + k * fb, d.data_ptr() + (k + 1) * fb, w, h, fl.data_ptr(), _stream())
        out.append(fetch(fl))
    return np.stack(out)


@pytest.mark.parametrize("w,h", [(67, 45), (192, 128)])
@pytest.mark.parametrize("warps,median", [(0, 3), (1, 5), (2, 3)])
@pytest.mark.parametrize("chunk", [None, "2"])
def test_stream_flows_equal_the_pair_entry_point(nsc, monkeypatch, w, h, warps, median, chunk):
    import torch

    if chunk is None:
        monkeypatch.delenv("NUS_FLOW_MAX_CHUNK_PAIRS", raising=False)
    else:
        monkeypatch.setenv("NUS_FLOW_MAX_CHUNK_PAIRS", chunk)  # 4 pairs in chunks of 2 + 2
    n = 5
    frames = _sequence(w, h, n)
    d = put(frames, "cuda:0")
    want = _pair_flows(nsc, d, n, w, h, warps, median)
    assert float(np.abs(want).max()) > 1.5  # motion of more than a pixel
    # ... which is the restatement, and the host entry point's
    want0 = M.estimate_f32(oracle, frames[0], frames[1], warps=warps, median=median, **P)
    _assert_values(want[0], want0, ("estimate_device", w, h, warps, median))
    _assert_values(_estimator(nsc, warps, median).estimate(frames[0], frames[1], w, h), want[0], ("estimate", w, h, warps, median))
    for mode, tiled in (("exact", 0), ("exact", 1), ("exact", 2), ("exact", 3), ("fast", 1), ("fast", 3)):
        flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
        _estimator(nsc, warps, median, mode, tiled).estimate_device_stream(d.data_ptr(), n, w, h, flows.data_ptr(), _stream())
        got = fetch(flows)
        if mode == "exact":
            _assert_values(got, want, ("estimate_device_stream", w, h, warps, median, tiled, chunk))
            continue
        for k in range(n - 1):
            dist = float(np.abs(got[k].astype(np.float64) - want[k]).max())
            bound = FAST_CONTRACT
            if dist > bound:
                f64 = M.estimate(frames[k], frames[k + 1], warps=warps, median=median, **P)
                d64 = float(np.abs(want[k] - f64).max())
                bound = max(bound, FAST_CONDITIONING * d64)
                print(f"FAST median stream beyond 1e-3 px | {w}x{h} pair {k} | warps {warps} median {median} tiled {tiled} | {dist:.2e} | f32 from f64 {d64:.2e}")
            assert dist <= bound, (w, h, warps, median, tiled, k, dist)
    assert np.array_equal(fetch(d), frames)  # the frames are inputs


@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("mode,tiled", [("exact", 1), ("exact", 0), ("fast", 3)])
def test_interpolating_entry_points_equal_estimate_then_warp(nsc, ffmt, mode, tiled):
    import torch

    w, h, n = 192, 128, 5
    warps, median = 1, 5
    times = [0.25, 0.5, 0.75]
    frames = _sequence(w, h, n)
    d = put(frames, "cuda:0")
    fb = w * h * 4
    fdt = torch.float32 if ffmt == "f32" else torch.float16
    s = _stream()
    f32 = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    _estimator(nsc, warps, median, mode, tiled).estimate_device_stream(d.data_ptr(), n, w, h, f32.data_ptr(), s)
    f32 = fetch(f32)
    assert float(np.abs(f32).max()) > 1.5
    want_flows = f32 if ffmt == "f32" else f32.astype(np.float16)
    d_flows = put(want_flows, "cuda:0")
    warp = nsc.WgpuFrameInterpolator()
    warp.set_mode("fma")
    warp.set_flow_format(ffmt)
    want_multi = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
    warp.interpolate_multi_device(d.data_ptr(), fb, d.data_ptr() + fb, fb, d_flows.data_ptr(), w, h, times, want_multi.data_ptr(), 0, n - 1, s)
    want_one = guarded.empty((n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
    warp.interpolate_device(d.data_ptr(), fb, d.data_ptr() + fb, fb, d_flows.data_ptr(), w, h, 0.5, want_one.data_ptr(), n - 1, s)
    want_multi, want_one = fetch(want_multi), fetch(want_one)
    assert np.array_equal(want_multi[:, 1], want_one)
    for with_flows in (True, False):
        fe = _estimator(nsc, warps, median, mode, tiled)
        flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=fdt, device="cuda:0")
        mid = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
        fe.interpolate_multi_device_stream(d.data_ptr(), n, w, h, times, mid.data_ptr(), flows.data_ptr() if with_flows else 0, 0, s, flow_format=ffmt)
        assert np.array_equal(fetch(mid), want_multi), (ffmt, mode, tiled, with_flows, "multi")
        if with_flows:
            assert np.array_equal(fetch(flows), want_flows), (ffmt, mode, tiled, "multi flows")
        else:
            assert np.isnan(fetch(flows).astype(np.float32)).all()  # nothing was stored there
        flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=fdt, device="cuda:0")
        one = guarded.empty((n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
        fe.interpolate_device_stream(d.data_ptr(), n, w, h, 0.5, one.data_ptr(), flows.data_ptr() if with_flows else 0, s, ffmt)
        assert np.array_equal(fetch(one), want_one), (ffmt, mode, tiled, with_flows, "single")
        if with_flows:
            assert np.array_equal(fetch(flows), want_flows), (ffmt, mode, tiled, "single flows")
    assert np.array_equal(fetch(d), frames)


# ---- off means off -----------------------------------------------------------------------------------------------------------------
def test_median_zero_after_median_five_equals_a_fresh_handle(nsc):
    import torch

    w, h, n = 192, 128, 4
    frames = _sequence(w, h, n)
    d = put(frames, "cuda:0")
    for mode, tiled in (("exact", 1), ("fast", 3)):
        used, fresh = _estimator(nsc, 1, 5, mode, tiled), _estimator(nsc, 1, 0, mode, tiled)
        out, workspace = {}, {}
        for name, fe in (("used", used), ("fresh", fresh)):
            if name == "used":  # one pair and one stream with the median on, then off
                scratch = guarded.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda:0")
                assert fe.estimate(frames[0], frames[1], w, h).shape == (h, w, 2)
                fe.estimate_device_stream(d.data_ptr(), n, w, h, scratch.data_ptr(), _stream())
                torch.cuda.synchronize()
                fe.set_median(0)
            assert fe.median_size == 0 and fe.warps == 1
            flows = guarded.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda:0")
            fe.estimate_device_stream(d.data_ptr(), n, w, h, flows.data_ptr(), _stream())
            mid = guarded.empty((n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
            half = guarded.empty((n - 1, h, w, 2), dtype=torch.float16, device="cuda:0")
            fe.interpolate_device_stream(d.data_ptr(), n, w, h, 0.5, mid.data_ptr(), half.data_ptr(), _stream(), "f16")
            torch.cuda.synchronize()  # (the host entry point runs on the handle's own stream, in the same workspace)
            out[name] = (fe.estimate(frames[0], frames[1], w, h), fetch(flows), fetch(mid), fetch(half))
            workspace[name] = fe.workspace_bytes
        for x, y in zip(out["used"], out["fresh"]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), mode  # bytes: no median ran
        assert workspace["used"] == workspace["fresh"] > 0, (mode, workspace)  # the median reserved nothing of its own
        if mode == "exact":  # and median = 0 is the estimator _flow_warp64 restates
            assert np.array_equal(out["fresh"][0].view(np.uint32), W.estimate_f32(oracle, frames[0], frames[1], warps=1, **P).view(np.uint32))


# ---- what it is for ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [W.ROWS[0], W.ROWS[5]], ids=lambda r: f"pan{r[2]}mv{r[3]}".replace(" ", ""))
def test_in_between_frame_is_nearer_the_true_one(nsc, row):
    w, h = row[:2]
    a, b, true_mid = W.scene(row)
    psnr = {}
    for median in (0, 5):
        it = nsc.PyFrameInterpolator("optical_flow", flow_warps=1, flow_median=median)
        it.initialize(w, h)
        got = np.frombuffer(it.interpolate(a.tobytes(), b.tobytes(), 0.5), np.uint8).reshape(h, w, 4)
        psnr[median] = scenes.psnr_rgb(got, true_mid)
    print(f"{row}: flow_warps 1, flow_median 0 {psnr[0]:.2f} dB, flow_median 5 {psnr[5]:.2f} dB")
    assert psnr[5] >= psnr[0] + 0.3  # the CPU yardstick's margin for 5 x 5 at warps 1 on the wide rows


def test_step_motion_takes_the_setting(nsc):
    import torch

    w, h, n = 192, 128, 3
    frames = _sequence(w, h, n + 1)
    dev = torch.device("cuda:0")
    d = put(frames, "cuda:0")
    s = _stream()
    pipe = nsc.FramePipeline(w, h, 2, "lanczos3", 0.5, lanczos_mode="exact")
    want = {}
    for median in (0, 3):
        fl = guarded.empty((n, h, w, 2), dtype=torch.float32, device=dev)
        _estimator(nsc, 1, median).estimate_device_stream(d.data_ptr(), n + 1, w, h, fl.data_ptr(), s)
        want[median] = fetch(fl)
    assert float(np.abs(want[3] - want[0]).max()) > 0.05
    for median in (3, 0, 3):
        mid, up_real, up_mid = guarded.like(pipe.alloc(n, dev))
        flows = guarded.empty((n, h, w, 2), dtype=torch.float32, device=dev)
        pipe.step_motion(d, flows, mid, up_real, up_mid, s, flow_warps=1, flow_median=median)
        assert np.array_equal(fetch(flows), want[median]), median
        for k in range(n):
            assert np.array_equal(fetch(mid[k]), oracle.warp_blend(frames[k], frames[k + 1], want[median][k], 0.5)), (median, k)
    with pytest.raises(ValueError, match="median"):
        pipe.step_motion(d, flows, mid, up_real, up_mid, s, flow_warps=1, flow_median=4)
