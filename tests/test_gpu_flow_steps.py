"""Every steps-per-launch instantiation of the Horn-Schunck Jacobi kernels that launch_hs_iterate can reach, run on the GPU: one
case per row of tests/_hs_steps.py CASES (tests/test_flow_steps_census.py holds that table against the kernels the library is
built with).  K is the kernel's geometry -- a streamed strip is 64 - 2K columns wide, a row block carries K halo rows per side, an
LDS tile a K-cell halo, the delay lines and rings are K deep -- so the sizes sit at the seams of the row's K.  EXACT kernels: the
oracle's bits.  FAST kernels: nus_flow_set_mode's 1e-3 px against the oracle, the ring form bit for bit the shifting form."""
import numpy as np
import pytest

import _hs_steps as hs
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

LAM = 4e-4


def _params(group):
    return pytest.mark.parametrize("case", hs.group(group), ids=lambda c: c.id)


def _smooth(w, h, shift=0.0):
    """The smooth textured RGBA8 frame of tests/test_flow.py, its content displaced by `shift` pixels in x."""
    x = np.arange(w, dtype=np.float64)[None, :] - shift
    y = np.arange(h, dtype=np.float64)[:, None]
    v = 127.5 + 45 * np.sin(x / 3.0) * np.cos(y / 4.0) + 50 * np.sin((x + 2 * y) / 23.0) + 25 * np.sin(x / 9.0 + y / 11.0)
    img = np.empty((h, w, 4), np.uint8)
    img[..., 0] = np.clip(v, 0, 255)
    img[..., 1] = np.clip(255 - v, 0, 255)
    img[..., 2] = np.clip(v * 0.5 + 40, 0, 255)
    img[..., 3] = 255
    return img


_memo = {}


def _once(key, make):
    """A reference computed once and shared between the cases that need it (handed out read-only)."""
    if key not in _memo:
        v = make()
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
        _memo[key] = v
    return _memo[key]


def _frames(oracle_mod, content, w, h, n):
    """n RGBA8 frames: "noise" -- frame k is noise frame k mod 8, so a long stream has eight distinct pairs; "smooth" -- the moving
    pattern with +-3 of sensor noise on top, as in the 1080p FAST contract test."""
    def make():
        if content == "noise":
            base = [oracle_mod.gen_noise(w, h, 700 + k) for k in range(8)]
            return np.stack([base[k % 8] for k in range(n)])
        rng = np.random.default_rng(7)
        out = np.stack([_smooth(w, h, 1.75 * k) for k in range(n)])
        out[..., :3] = np.clip(out[..., :3].astype(np.int16) + rng.integers(-3, 4, size=(n, h, w, 3)), 0, 255).astype(np.uint8)
        return out
    return _once(("frames", content, w, h, n), make)


def _want_flows(oracle_mod, case):
    """The oracle's flow of every distinct pair of the case's stream: pair k's is element k mod 8."""
    frames = _frames(oracle_mod, case.content, case.w, case.h, case.frames)
    distinct = min(case.frames - 1, 8 if case.content == "noise" else case.frames - 1)
    return _once(("flows", case.content, case.w, case.h, distinct, case.levels, case.coarse, case.refine), lambda: [
        oracle_mod.flow_estimate(frames[k], frames[k + 1], case.levels, case.coarse, case.refine, LAM) for k in range(distinct)])


def _estimator(nsc, case):
    fe = nsc.FlowEstimator(levels=case.levels, coarse_iterations=case.coarse, refine_iterations=case.refine, lambda_=LAM)
    fe.set_mode(case.mode)
    fe.set_tiled(case.tiled)
    return fe


def _stream_flows(fe, d_frames, case):
    import torch

    n, w, h = case.frames, case.w, case.h
    d_flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device=d_frames.device)
    fe.estimate_device_stream(d_frames.data_ptr(), n, w, h, d_flows.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_flows


@pytest.mark.gpu
@pytest.mark.parametrize("case", hs.group("a") + hs.group("b"), ids=lambda c: c.id)
def test_horn_schunck_primitive_every_steps_per_launch(nsc, oracle_mod, case):
    """a, b: the coefficient-plane kernels behind FlowEstimator.horn_schunck -- k_hs_stream<K, false, false> at one strip, the first
    column of a second and of a third strip, one and two row blocks; k_hs_tiled<16, K, 1024> at one tile, one cell past it, ragged --
    from zero flow and from a random start, and a step count whose launches differ in K (the result ends in the other buffer)."""
    w, h = case.w, case.h
    i1 = _once(("f32", w, h, 5), lambda: oracle_mod.rgba8_to_f32(oracle_mod.gen_noise(w, h, 5)))
    i2 = _once(("f32", w, h, 6), lambda: oracle_mod.rgba8_to_f32(oracle_mod.gen_noise(w, h, 6)))
    f0 = _once(("start", w, h), lambda: np.random.default_rng(w * h).standard_normal((h, w, 2)).astype(np.float32))
    fe = _estimator(nsc, case)
    for fin in (None, f0):
        want = _once(("hs", w, h, fin is None, case.coarse), lambda: oracle_mod.horn_schunck(i1, i2, fin, iterations=case.coarse, lam=LAM))
        got = fe.horn_schunck(i1, i2, fin, iterations=case.coarse, lambda_=LAM)
        assert np.array_equal(got, want), (case.id, "zero start" if fin is None else "random start", int((got != want).sum()))


@pytest.mark.gpu
@_params("c")
def test_tiled_mid_and_big_every_steps_per_launch(nsc, oracle_mod, case):
    """c: k_hs_tiled<32, K, 1024> (18 pairs of 130 x 70: 270 tiles) and k_hs_tiled<32, K, 256> (69 pairs: 1035 tiles) through the
    batch path; every pair's flow against its own reference, so the pair index on the grid's z axis is held too."""
    frames = _frames(oracle_mod, "noise", case.w, case.h, case.frames)
    want = _want_flows(oracle_mod, case)
    got = fetch(_stream_flows(_estimator(nsc, case), put(frames), case))
    wrong = [k for k in range(case.frames - 1) if not np.array_equal(got[k], want[k % 8])]
    assert not wrong, (case.id, wrong)


@pytest.mark.gpu
@_params("d")
def test_streamed_plane_forms_every_steps_per_launch(nsc, oracle_mod, case):
    """d: k_hs_stream<K, true, false> (the coarsest level: null-input first launch) and the upsampling k_hs_stream<K, true, true>
    through the batch path, at the strip seams of K; the pair entry -- coefficient planes -- gives the stream's flow 1 bit for bit."""
    import torch

    w, h = case.w, case.h
    frames = _frames(oracle_mod, "noise", w, h, case.frames)
    want = _want_flows(oracle_mod, case)
    fe = _estimator(nsc, case)
    d_frames = put(frames)
    got = fetch(_stream_flows(fe, d_frames, case))
    for k in range(case.frames - 1):
        assert np.array_equal(got[k], want[k]), (case.id, k, int((got[k] != want[k]).sum()))
    one = guarded.full((h, w, 2), float("nan"), dtype=torch.float32, device=d_frames.device)
    fe.estimate_device(d_frames[1].data_ptr(), d_frames[2].data_ptr(), w, h, one.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(fetch(one), got[1]), (case.id, "a pair alone = the same pair inside a stream")


@pytest.mark.gpu
@_params("e")
def test_fast_every_steps_per_launch(nsc, oracle_mod, case, monkeypatch):
    """e: k_hs_stream_fast<K, UPS, RING>, K = 1..8 without and K = 1..5, 7, 8 with the upsampling first launch.  Within the 1e-3 px
    of nus_flow_set_mode's contract (nuscaler_hip.h) of the oracle's flow; not the oracle's bits (the FAST kernels ran); the ring
    form bit for bit the shifting form (NUS_HS_FAST_SHIFT, read per call)."""
    frames = _frames(oracle_mod, case.content, case.w, case.h, case.frames)
    want = _want_flows(oracle_mod, case)
    fe = _estimator(nsc, case)
    d_frames = put(frames)
    got = {}
    for form in ("ring", "shift"):
        if form == "shift":
            monkeypatch.setenv("NUS_HS_FAST_SHIFT", "1")
        else:
            monkeypatch.delenv("NUS_HS_FAST_SHIFT", raising=False)
        got[form] = fetch(_stream_flows(fe, d_frames, case))
    monkeypatch.delenv("NUS_HS_FAST_SHIFT", raising=False)
    ring = got["ring"]
    dist = [float(np.abs(ring[k].astype(np.float64) - want[k].astype(np.float64)).max()) for k in range(case.frames - 1)]
    print(f"{case.id}: |FAST - oracle| = " + ", ".join(f"{d:.3e}" for d in dist) + f" px, max |flow| = {max(float(np.abs(f).max()) for f in want):.2f} px")
    assert np.isfinite(ring).all(), case.id
    assert max(dist) <= 1e-3, (case.id, dist)
    assert any(not np.array_equal(ring[k], want[k]) for k in range(case.frames - 1)), (case.id, "the FAST kernels did not run")
    assert np.array_equal(ring, got["shift"]), (case.id, int((ring != got["shift"]).sum()))


@pytest.mark.gpu
@_params("f")
def test_fast_rg16float_handoff_every_last_launch(nsc, oracle_mod, case):
    """f: the level's last FAST launch stores the flow as Rg16Float itself, K = 1..4 (upsampling first launch = last launch) and
    K = 6.  The halves are the f32 flows of estimate_device_stream rounded to nearest even, bit for bit, nothing behind them is
    written, and the in-between frames are the FMA-mode warp's on those halves."""
    import torch

    n, w, h, t = case.frames, case.w, case.h, 0.5
    d_frames = put(_frames(oracle_mod, case.content, w, h, n))
    s = torch.cuda.current_stream().cuda_stream
    fe = _estimator(nsc, case)
    want16 = _stream_flows(fe, d_frames, case).to(torch.float16)
    it = nsc.WgpuFrameInterpolator()
    it.set_mode("fma")
    it.set_flow_format("f16")
    fb = w * h * 4
    want_mid = guarded.zeros((n - 1, h, w, 4), dtype=torch.uint8, device=d_frames.device)
    it.interpolate_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, want16.data_ptr(), w, h, t, want_mid.data_ptr(), n - 1, s)
    cells = (n - 1) * h * w
    buf = guarded.full((2 * cells, 2), 1234.0, dtype=torch.float16, device=d_frames.device)  # 4 bytes per cell, as much again behind
    got16 = buf[:cells].view(n - 1, h, w, 2)
    got16.fill_(float("nan"))
    got_mid = guarded.full((n - 1, h, w, 4), 0xAB, dtype=torch.uint8, device=d_frames.device)
    fe.interpolate_device_stream(d_frames.data_ptr(), n, w, h, t, got_mid.data_ptr(), got16.data_ptr(), s, "f16")
    torch.cuda.synchronize()
    assert bool((buf[cells:] == 1234.0).all()), (case.id, "wrote past the f16 flows")
    assert torch.equal(got16.view(torch.int16), want16.view(torch.int16)), case.id
    assert torch.equal(got_mid, want_mid), case.id
