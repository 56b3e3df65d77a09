"""The select warp on the GPU (nus_interp_interpolate_select_device, nus_interp_interpolate_select, nus_flow_set_bidirectional):
EXACT frames byte for byte against the float32 restatement (tests/_flow_select.py), R = -F against the plain warp, FMA pixels
under the warp contract with one of the two candidates and with the restatement's choice where it is decided, the estimator's
interpolating entry points with the setting on against estimate both ways followed by the select warp, off after on against
fresh handles, scene detection on top, and what it is for: the in-between frame on scenes with a known true mid-frame.  Every
device output comes from conftest.guarded."""
import functools

import numpy as np
import pytest

import _bm_bidir as scenes
import _flow_select as S
import _flow_warp64 as W
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

P = W.PARAMS
TABLE = (P["levels"], P["coarse_iters"], P["refine_iters"])
FMA_POSITION_ULPS = 0.5  # the FMA-mode warp's sample position is one fused multiply-add (tests/test_gpu_warp_fma_contract.py)
# An FMA sample is within one count of the EXACT one: two counts per channel difference, six per error, twelve on the difference of
# two errors.  Beyond that the FMA kernel's choice must be the restatement's.
DECIDED_MARGIN = 12
UNDECIDED_CAP = 0.15  # the share of pixels within the margin (8.5 - 9.9 % on these inputs, from the restatement): a cap, not a measurement
BIG = [(67, 45), (130, 70)]  # odd width: one pixel per thread; even width: a pair per thread, more than one block each way
TINY = [(2, 2), (1, 1), (5, 1), (1, 7)]  # 2 x 2: the smallest tile frame; the others: the one-pixel-per-thread kernels
TIMES3 = [float(np.float32(0.25)), 0.5, float(np.float32(0.7))]


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


# ---- the CPU inputs and references: once per module run, read-only -------------------------------------------------------------------
def _smooth(rng, w, h):
    coarse = (rng.random((h // 8 + 2, w // 8 + 2, 2)) - 0.5) * 24  # +-12 px
    yy, xx = np.mgrid[0:h, 0:w]
    y0, x0, fy, fx = yy // 8, xx // 8, (yy % 8 / 8.0)[..., None], (xx % 8 / 8.0)[..., None]
    return ((coarse[y0, x0] * (1 - fx) + coarse[y0, x0 + 1] * fx) * (1 - fy)
            + (coarse[y0 + 1, x0] * (1 - fx) + coarse[y0 + 1, x0 + 1] * fx) * fy).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _flows(w, h):
    """(F, R), each (3, h, w, 2) float32 -- three different pairs of flows for three pairs of frames: smooth +-12 px / an
    independent smooth field; a motion boundary (sub-pixel parts included) / smooth; vectors that leave the frame / smooth."""
    rng = np.random.default_rng(8001 + 31 * w + h)
    step = np.full((h, w, 2), (-3.25, 1.5), np.float32)
    step[h // 2:, w // 2:] = (7.5, -2.75)
    outside = ((rng.random((h, w, 2)) - 0.5) * 6).astype(np.float32)
    outside[::3, 1::2] += (2.0 * w + 0.5, -1.5 * h - 0.25)
    outside[1::3, ::2] -= (1.25 * w, -3.0 * h)
    F = np.stack([_smooth(rng, w, h), step, outside])
    R = np.stack([_smooth(rng, w, h) for _ in range(3)])
    F.setflags(write=False), R.setflags(write=False)
    return F, R


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    f = np.random.default_rng(8101 + 31 * w + h).integers(0, 256, (4, h, w, 4), dtype=np.uint8)  # uniform noise
    f.setflags(write=False)
    return f


def _as_read(flows, ffmt):
    return flows if ffmt == "f32" else flows.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _want(w, h, ffmt, t, rounds, bgra=False):
    """The restatement for the three pairs of a size, from the flows as the warp reads them: (frames, picked_backward, eF, eR)."""
    frames = _frames(w, h)
    if bgra:
        frames = frames[..., [2, 1, 0, 3]]
    F, R = (_as_read(f, ffmt) for f in _flows(w, h))
    out = [S.select_f32(np.ascontiguousarray(frames[i]), np.ascontiguousarray(frames[i + 1]), F[i], R[i], t, rounds) for i in range(3)]
    out = tuple(np.stack([o[k] for o in out]) for k in range(4))
    for o in out:
        o.setflags(write=False)
    return out


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
    return it


def _device_flows(w, h, ffmt):
    return tuple(put(np.ascontiguousarray(f if ffmt == "f32" else f.astype(np.float16))) for f in _flows(w, h))


def _select(it, d_frames, d_fwd, d_bwd, w, h, times, n=3, gap=0):
    """-> (n, len(times), h, w, 4); gap: that many frames of room behind every pair's frames (out_pair_stride), checked untouched."""
    import torch

    fb = w * h * 4
    k = len(times)
    out = guarded.full((n, k + gap, h, w, 4), 0xA5, dtype=torch.uint8, device="cuda:0")
    it.interpolate_select_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_fwd.data_ptr(), d_bwd.data_ptr(), w, h, times,
                                 out.data_ptr(), (k + gap) * fb if gap else 0, n, _stream())
    got = fetch(out)
    assert (got[:, k:] == 0xA5).all()  # nothing stored into the gap
    return got[:, :k]


# ---- EXACT: byte for byte the restatement -------------------------------------------------------------------------------------------
# three pairs with three different pairs of flows: a kernel that reads pair 0's plane for pair 2 shows up as wrong bytes
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", BIG + TINY)
def test_exact_device_entry_point(nsc, w, h, ffmt):
    d_frames = put(np.ascontiguousarray(_frames(w, h)))
    d_fwd, d_bwd = _device_flows(w, h, ffmt)
    for rounds in (0, 1, 3):
        it = _interp(nsc, rounds, "exact", ffmt)
        single = _select(it, d_frames, d_fwd, d_bwd, w, h, [0.5])
        _assert_bytes(single[:, 0], _want(w, h, ffmt, 0.5, rounds)[0], ("select, one time", w, h, ffmt, rounds))
        multi = _select(it, d_frames, d_fwd, d_bwd, w, h, TIMES3, gap=1 if rounds == 1 else 0)
        for k, t in enumerate(TIMES3):
            _assert_bytes(multi[:, k], _want(w, h, ffmt, t, rounds)[0], ("select, three times", w, h, ffmt, rounds, t))
        assert np.array_equal(multi[:, 1], single[:, 0])
        if (w, h) in BIG:  # both branches and the tie rule are exercised
            _, back, eF, eR = _want(w, h, ffmt, 0.5, rounds)
            share, ties = float(back.mean()), float((eF == eR).mean())
            print(f"select {w}x{h} {ffmt} rounds {rounds}: backward at {share:.3f} of the pixels, ties at {ties:.4f}")
            assert 0.3 < share < 0.6 and ties > 0.0


@pytest.mark.parametrize("w,h", BIG)
def test_exact_bgra_input(nsc, w, h):
    d_frames = put(np.ascontiguousarray(_frames(w, h)))
    d_fwd, d_bwd = _device_flows(w, h, "f32")
    got = _select(_interp(nsc, 1, "exact", "f32", "bgra"), d_frames, d_fwd, d_bwd, w, h, TIMES3)
    for k, t in enumerate(TIMES3):
        want, back = _want(w, h, "f32", t, 1, True)[:2]
        _assert_bytes(got[:, k], want, ("bgra select", w, h, t))
        assert np.array_equal(back, _want(w, h, "f32", t, 1)[1])  # the error is symmetric in R and B: the same choice


@pytest.mark.parametrize("w,h", [(67, 45), (5, 1)])
def test_exact_host_entry_point(nsc, w, h):
    frames, (F, R) = _frames(w, h), _flows(w, h)
    it = _interp(nsc, 3)
    for i in range(3):
        got = it.interpolate_select_multi_py(frames[i].tobytes(), frames[i + 1].tobytes(), w, h, F[i], R[i], times=TIMES3)
        for k, t in enumerate(TIMES3):
            _assert_bytes(np.frombuffer(got[k], np.uint8).reshape(h, w, 4), _want(w, h, "f32", t, 3)[0][i], ("host select", w, h, t, i))
        one = it.interpolate_select_py(frames[i].tobytes(), frames[i + 1].tobytes(), w, h, F[i], R[i])
        assert one == got[1]
    # the plain host call behind it, on the same handle: one flow, the old bytes
    import oracle
    import _flow_project as PJ

    got = np.frombuffer(it.interpolate_py(frames[0].tobytes(), frames[1].tobytes(), w, h, time_t=0.5, flow=F[0]), np.uint8).reshape(h, w, 4)
    _assert_bytes(got, oracle.warp_blend(frames[0], frames[1], PJ.project_f32(F[0], 0.5, 3), 0.5), ("host plain", w, h))


# ---- R = -F, rounds 0: every pixel a tie, the plain warp's bytes ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "fma"])
@pytest.mark.parametrize("w,h", BIG + [(5, 1)])
def test_negated_forward_flow_is_the_plain_warp(nsc, w, h, mode):
    import torch

    F = _flows(w, h)[0]
    d_frames, d_fwd, d_bwd = put(np.ascontiguousarray(_frames(w, h))), put(np.ascontiguousarray(F)), put(np.ascontiguousarray(-F))
    it = _interp(nsc, 0, mode)
    got = _select(it, d_frames, d_fwd, d_bwd, w, h, TIMES3)
    fb = w * h * 4
    want = guarded.empty((3, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
    it.interpolate_multi_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_fwd.data_ptr(), w, h, TIMES3, want.data_ptr(), 0, 3,
                                _stream())
    _assert_bytes(got, fetch(want), ("R = -F", w, h, mode))


# ---- FMA: each pixel under the warp contract with one of the candidates, the restatement's where that is decided --------------------------
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", BIG)
def test_fma_pixels_meet_the_warp_contract_with_a_candidate(nsc, w, h, ffmt):
    frames = _frames(w, h)
    d_frames = put(np.ascontiguousarray(frames))
    d_fwd, d_bwd = _device_flows(w, h, ffmt)
    F, R = (_as_read(f, ffmt) for f in _flows(w, h))
    for rounds in (0, 3):
        it = _interp(nsc, rounds, "fma", ffmt)
        multi = _select(it, d_frames, d_fwd, d_bwd, w, h, TIMES3)
        assert np.array_equal(multi[:, 1], _select(it, d_frames, d_fwd, d_bwd, w, h, [0.5])[:, 0])
        for k, t in enumerate(TIMES3):
            _, back, eF, eR = _want(w, h, ffmt, t, rounds)
            undecided = 0
            for i in range(3):
                gF, gR = S.candidates_f32(F[i], R[i], t, rounds)
                ok_f = S.contract_pixels(multi[i, k], frames[i], frames[i + 1], gF, t, FMA_POSITION_ULPS)
                ok_r = S.contract_pixels(multi[i, k], frames[i], frames[i + 1], gR, t, FMA_POSITION_ULPS)
                assert (ok_f | ok_r).all(), (w, h, ffmt, rounds, t, i, int((~(ok_f | ok_r)).sum()), np.argwhere(~(ok_f | ok_r))[:4].tolist())
                decided = np.abs(eF[i] - eR[i]) > DECIDED_MARGIN
                ok_choice = np.where(back[i], ok_r, ok_f)
                assert ok_choice[decided].all(), (w, h, ffmt, rounds, t, i, np.argwhere(decided & ~ok_choice)[:4].tolist())
                undecided += int((~decided).sum())
            share = undecided / (3 * w * h)
            print(f"FMA select {w}x{h} {ffmt} rounds {rounds} t {t}: within {DECIDED_MARGIN} of a tie {share:.4f}")
            assert share <= UNDECIDED_CAP


# ---- the estimator with the setting on ---------------------------------------------------------------------------------------------
def _estimator(nsc, mode, tiled, bidirectional, warps=1, median=3, project=2):
    fe = nsc.FlowEstimator(TABLE[0], TABLE[1], TABLE[2], P["lam"], warps=warps, median=median, project=project, bidirectional=bidirectional)
    fe.set_mode(mode)
    fe.set_tiled(tiled)
    assert fe.bidirectional == bidirectional
    return fe


def _stream_call(fe, d, n, w, h, ffmt, with_flows=True):
    import torch

    fdt = torch.float32 if ffmt == "f32" else torch.float16
    flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=fdt, device="cuda:0")
    mid = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
    fe.interpolate_multi_device_stream(d.data_ptr(), n, w, h, TIMES3, mid.data_ptr(), flows.data_ptr() if with_flows else 0, 0, _stream(),
                                       flow_format=ffmt)
    return fetch(mid), fetch(flows)


# the FAST batch path and the EXACT pair-by-pair (shader-shaped) path
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("mode,tiled", [("fast", 1), ("exact", 0), ("exact", 1)])
def test_estimator_frames_equal_estimates_both_ways_then_select_warp(nsc, monkeypatch, mode, tiled, ffmt):
    import torch

    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    w, h, n = 67, 45, 4
    frames = W.lattice_frames(w, h, n)
    d = put(frames, "cuda:0")
    fb = w * h * 4
    s = _stream()
    est = _estimator(nsc, mode, tiled, False)
    fwd = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    bwd = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    for k in range(n - 1):
        a, b = d.data_ptr() + k * fb, d.data_ptr() + (k + 1) * fb
        est.estimate_device(a, b, w, h, fwd.data_ptr() + k * w * h * 8, s)
        est.estimate_device(b, a, w, h, bwd.data_ptr() + k * w * h * 8, s)
    fwd, bwd = fetch(fwd), fetch(bwd)
    assert float(np.abs(fwd).max()) > 1.5 and float(np.abs(fwd + bwd).max()) > 0.25  # motion, and the two estimates are not mirror images
    cast = (lambda f: f) if ffmt == "f32" else (lambda f: f.astype(np.float16))
    warp = _interp(nsc, 2, "fma", ffmt)
    want = guarded.empty((n - 1, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
    d_fwd, d_bwd = put(cast(fwd)), put(cast(bwd))
    warp.interpolate_select_device(d.data_ptr(), fb, d.data_ptr() + fb, fb, d_fwd.data_ptr(), d_bwd.data_ptr(), w, h, TIMES3, want.data_ptr(), 0,
                                   n - 1, s)
    want = fetch(want)
    off_mid, off_flows = _stream_call(_estimator(nsc, mode, tiled, False), d, n, w, h, ffmt)
    assert not np.array_equal(off_mid, want)  # the setting does something here
    fe = _estimator(nsc, mode, tiled, True)
    mid, flows = _stream_call(fe, d, n, w, h, ffmt)
    _assert_bytes(mid, want, ("bidirectional stream", mode, tiled, ffmt))
    assert np.array_equal(flows.view(np.uint8), off_flows.view(np.uint8))  # d_flows: the forward flows, the bytes of the setting off
    assert np.array_equal(flows.view(np.uint8), cast(fwd).view(np.uint8))
    # no flows wanted: the same frames; and the workspace poisoned between two identical calls: the same frames again
    mid2, untouched = _stream_call(fe, d, n, w, h, ffmt, with_flows=False)
    _assert_bytes(mid2, want, ("bidirectional stream, no d_flows", mode, tiled, ffmt))
    assert np.isnan(untouched.astype(np.float32)).all()
    fe._fill_workspace(0xFF, s)
    _assert_bytes(_stream_call(fe, d, n, w, h, ffmt, with_flows=False)[0], want, ("bidirectional stream, poisoned workspace", mode, tiled, ffmt))
    # the single-time entry point is frame 1 of the set
    one = guarded.empty((n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
    fe.interpolate_device_stream(d.data_ptr(), n, w, h, 0.5, one.data_ptr(), 0, s, ffmt)
    _assert_bytes(fetch(one), want[:, 1], ("bidirectional stream, one time", mode, tiled, ffmt))
    assert np.array_equal(fetch(d), frames)  # the frames are inputs


# ---- off means off -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tiled", [("fast", 1), ("exact", 0), ("exact", 1), ("exact", 2), ("exact", 3), ("fast", 3)])
def test_off_after_on_equals_a_fresh_handle(nsc, mode, tiled):
    import torch

    w, h, n = 67, 45, 4
    d = put(W.lattice_frames(w, h, n), "cuda:0")
    s = _stream()
    out, workspace = {}, {}
    for name in ("used", "fresh"):
        fe = _estimator(nsc, mode, tiled, name == "used")
        if name == "used":  # calls with the setting on, then off
            _stream_call(fe, d, n, w, h, "f32")
            _stream_call(fe, d, n, w, h, "f16")
            torch.cuda.synchronize()
            assert fe.workspace_bytes > 0
            fe.set_bidirectional(False)
        assert fe.bidirectional is False
        out[name] = _stream_call(fe, d, n, w, h, "f32") + _stream_call(fe, d, n, w, h, "f16")
        est = guarded.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda:0")
        fe.estimate_device_stream(d.data_ptr(), n, w, h, est.data_ptr(), s)
        out[name] += (fetch(est),)
        torch.cuda.synchronize()
        workspace[name] = fe.workspace_bytes
    for x, y in zip(out["used"], out["fresh"]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), mode
    assert workspace["used"] == workspace["fresh"] > 0, (mode, workspace)  # turning the setting off gave its slots back


def test_existing_warp_unchanged_beside_the_select_warp(nsc):
    """One handle: the select warp, then the plain and the projecting warp -- the bytes of a handle that never ran the select warp."""
    w, h = 130, 70
    import torch

    d_frames = put(np.ascontiguousarray(_frames(w, h)))
    d_fwd, d_bwd = _device_flows(w, h, "f32")
    fb = w * h * 4
    for mode in ("exact", "fma"):
        for rounds in (0, 2):
            got = {}
            for name in ("used", "fresh"):
                it = _interp(nsc, rounds, mode)
                if name == "used":
                    _select(it, d_frames, d_fwd, d_bwd, w, h, TIMES3)
                out = guarded.empty((3, 3, h, w, 4), dtype=torch.uint8, device="cuda:0")
                it.interpolate_multi_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_fwd.data_ptr(), w, h, TIMES3, out.data_ptr(),
                                            0, 3, _stream())
                got[name] = fetch(out)
            assert np.array_equal(got["used"], got["fresh"]), (mode, rounds)


# ---- scene detection on top -----------------------------------------------------------------------------------------------------------
def test_scene_detection_still_repeats_the_flagged_pair(nsc):
    w, h, n = 67, 45, 4
    from nu_scaler_amd.synthetic import gradient_frame

    frames = W.lattice_frames(w, h, n).copy()
    for k in (2, 3):  # another shot: a cut between frames 1 and 2
        frames[k] = gradient_frame(w, h, k)
        frames[k, ..., 3] = 255
    det = nsc.SceneDetector()
    assert [bool(det.detect(frames[k], frames[k + 1], w, h)[0]) for k in range(n - 1)] == [False, True, False]
    d = put(np.ascontiguousarray(frames), "cuda:0")
    fe = _estimator(nsc, "exact", 1, True)
    fe.set_scene_detect(True)
    mid, _ = _stream_call(fe, d, n, w, h, "f32", with_flows=False)
    for k, t in enumerate(TIMES3):  # pair 1's frames are repeats of the nearer real frame
        _assert_bytes(mid[1, k], frames[1] if t < 0.5 else frames[2], ("cut pair", t))
    plain = _estimator(nsc, "exact", 1, True)
    want, _ = _stream_call(plain, d, n, w, h, "f32", with_flows=False)
    _assert_bytes(mid[[0, 2]], want[[0, 2]], "the other pairs: the select warp's frames")
    assert not np.array_equal(mid[1], want[1])


# ---- what it is for ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [1, 4], ids=lambda i: "{}x{}".format(*W.ROWS[i][:2]))
def test_in_between_frame_is_nearer_the_true_one(nsc, index):
    import torch

    row = W.ROWS[index]
    w, h = row[:2]
    a, b, true_mid = W.scene(row)
    d = put(np.ascontiguousarray(np.stack([a, b])), "cuda:0")
    psnr = {}
    for on in (False, True):
        fe = _estimator(nsc, "exact", 1, on, warps=2, median=5, project=3)
        mid = guarded.empty((1, h, w, 4), dtype=torch.uint8, device="cuda:0")
        fe.interpolate_device_stream(d.data_ptr(), 2, w, h, 0.5, mid.data_ptr(), 0, _stream(), "f32")
        psnr[on] = scenes.psnr_rgb(fetch(mid)[0], true_mid)
    table = S.MEASURED[2, 5, 3][index][2]
    print(f"{row}: warps 2, median 5, project 3: bidirectional off {psnr[False]:.2f} dB, on {psnr[True]:.2f} dB; the float64 witness's "
          f"selected cell {table:.2f} dB")
    assert psnr[True] >= psnr[False] - 0.05
    assert psnr[True] >= table - 0.3
