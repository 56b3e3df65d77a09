"""GPU: every way the FMA-mode warp (warp_blend_pixel<kWarpFma>, nus_warp_device.hpp) is reached, against the float64 contract
of tests/_warp64.py, at the smallest shapes where it can still go wrong.

interpolate_device and interpolate_multi_device, f32 and f16 flow: (64, 48) and (334, 117) run the 2 px/lane kernel (more than
one workgroup across, a ragged last block of 8 rows), (61, 7) and (333, 117) the 1 px/lane kernel (odd width, fewer rows than a
block), (1920, 64) the coordinates with the largest ulp the product meets; three pairs per call as a sliding stream; the time
sets [0.5], [0.25, 0.5, 0.75] and an irregular one with both ends.  An even width with a flow pointer that is pixel aligned but
not 16-byte aligned: the host entry accepts it (nus_checks.cpp asks for 8 / 4 bytes) and the dispatch sends it to the 1 px/lane
kernel.  Frames narrower or lower than 2 pixels run EXACT arithmetic in either mode: equal to the oracle.  BGRA / RGBX / BGRX
input: the witness runs on the converted frames.  BlockMatcher.warp_device from hand-made vectors at block sizes 8 / 16 / 32: at
dyadic times there is nothing to round, so FMA must equal EXACT byte for byte (tests/test_warp64_contract.py confirms it of the
emulation); at other times the contract.  One block-matching stream and one FlowEstimator.interpolate_device_stream call -- the
warp kernel behind the estimator and the warp inside the last Horn-Schunck launch -- checked with the vectors / flows the same
call returns.  Every case asserts a decided share of at least 0.9; the last test asserts that every entry was seen and prints,
per entry, samples, decided share and the share differing from the all-floor result.  Device outputs live in conftest.guarded
tensors and come down through nus_download."""
import functools

import numpy as np
import pytest

import _blockmatch as bmref
from _warp64 import edge_flow, warp_contract
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

MIN_DECIDED = 0.9
_STATS = {}  # entry -> [samples, decided, bytes differing from the all-floor result]
ENTRIES = ({f"{e} {k} {f}" for e in ("interpolate_device", "interpolate_multi_device") for k in ("2px/lane", "1px/lane") for f in ("f32", "f16")}
           | {f"{e} 1px/lane (flow pointer not 16-byte aligned) {f}" for e in ("interpolate_device", "interpolate_multi_device") for f in ("f32", "f16")}
           | {f"interpolate_multi_device {fmt}" for fmt in ("bgra", "rgbx", "bgrx")}
           | {"bm warp_device 2px/lane", "bm warp_device 1px/lane", "bm interpolate_stream_device", "flow interpolate_device_stream"})


def _f32(ts):
    return [float(np.float32(t)) for t in ts]


TIME_SETS = [_f32([0.5]), _f32([0.25, 0.5, 0.75]), _f32([0.0, 0.3, 1.0, 0.7])]


def _hold(entry, got, a, b, flow, t, tag, channels=(0, 1, 2, 3)):
    st = warp_contract(got, a, b, flow, t, 0.5, (entry,) + tuple(tag), channels=channels)
    s = _STATS.setdefault(entry, [0, 0, 0])
    s[0] += st["samples"]
    s[1] += st["decided"]
    s[2] += st["differ_from_floor"]
    share = st["decided"] / st["samples"]
    print(f"{entry} {tag}: samples {st['samples']}, decided {share:.4f}, differ from all-floor {st['differ_from_floor'] / st['samples']:.2e}")
    assert share >= MIN_DECIDED, (entry, tag, share)


@functools.lru_cache(maxsize=None)
def _frames(n, w, h):
    f = np.random.default_rng(6001 + 31 * w + h).integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    f.setflags(write=False)
    return f


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _interp(nsc, ffmt, fmt="rgba"):
    it = nsc.WgpuFrameInterpolator()
    it.set_mode("fma")
    it.set_flow_format(ffmt)
    it.set_input_format(fmt)
    return it


def _single(it, d_frames, flow_ptr, w, h, t, n_pairs):
    import torch

    fb = w * h * 4
    out = guarded.empty((n_pairs, h, w, 4), dtype=torch.uint8, device="cuda:0")
    it.interpolate_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, flow_ptr, w, h, t, out.data_ptr(), n_pairs, _stream())
    return fetch(out)


def _multi(it, d_frames, flow_ptr, w, h, times, n_pairs):
    import torch

    fb = w * h * 4
    out = guarded.empty((n_pairs, len(times), h, w, 4), dtype=torch.uint8, device="cuda:0")
    it.interpolate_multi_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, flow_ptr, w, h, times, out.data_ptr(), 0, n_pairs,
                                _stream())
    return fetch(out)


# (the widest case runs one single-time call instead of two: the witness of a 1920 x 64 frame takes 0.1 s)
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h,kernel", [(64, 48, "2px/lane"), (334, 117, "2px/lane"), (61, 7, "1px/lane"), (333, 117, "1px/lane"),
                                        (1920, 64, "2px/lane")])
def test_dense_flow_entries_meet_the_contract(nsc, w, h, kernel, ffmt):
    n = 3
    frames = _frames(n + 1, w, h)
    d_frames = put(np.ascontiguousarray(frames))
    it = _interp(nsc, ffmt)
    wide = w >= 1000
    for j, t in enumerate([0.3] if wide else [0.5, 0.3]):
        flow = edge_flow(n, w, h, t, 20 + j, kind="gauss" if j == 0 else "smooth")
        flow = flow if ffmt == "f32" else flow.astype(np.float16)
        d_flow = put(flow)  # (held until the frames are down: a temporary's memory would go to the next allocation)
        got = _single(it, d_frames, d_flow.data_ptr(), w, h, t, n)
        _hold(f"interpolate_device {kernel} {ffmt}", got, frames[:-1], frames[1:], flow, t, ((w, h), t))
    for j, times in enumerate(TIME_SETS):
        flow = edge_flow(n, w, h, times[min(1, len(times) - 1)], 30 + j)
        flow = flow if ffmt == "f32" else flow.astype(np.float16)
        d_flow = put(flow)
        got = _multi(it, d_frames, d_flow.data_ptr(), w, h, times, n)
        _hold(f"interpolate_multi_device {kernel} {ffmt}", got, frames[:-1], frames[1:], flow, times, ((w, h), tuple(times)))


@pytest.mark.parametrize("ffmt", ["f32", "f16"])
def test_even_width_with_an_unaligned_flow_pointer_takes_the_one_pixel_kernel(nsc, ffmt):
    """The flow field one vector into its allocation: 8 bytes (f32) / 4 bytes (f16) past a 16-byte boundary.  The entry points
    accept it (pointers must be pixel aligned, no more), xv_ok in nus_k_interp.hip is false and the 1 px/lane kernel runs on an
    even width.  Same arithmetic per pixel: the bytes of the aligned call, and the contract."""
    w, h, n = 64, 48, 3
    frames = _frames(n + 1, w, h)
    d_frames = put(np.ascontiguousarray(frames))
    it = _interp(nsc, ffmt)
    times = TIME_SETS[1]
    flow = edge_flow(n, w, h, 0.3, 40)
    flow = flow if ffmt == "f32" else flow.astype(np.float16)
    vector_bytes = 8 if ffmt == "f32" else 4
    shifted = np.concatenate([np.zeros((1, 2), flow.dtype), flow.reshape(-1, 2)])
    d_aligned, d_shifted = put(flow), put(shifted)
    assert d_aligned.data_ptr() % 16 == 0 and (d_shifted.data_ptr() + vector_bytes) % 16 == vector_bytes
    got = _single(it, d_frames, d_shifted.data_ptr() + vector_bytes, w, h, 0.3, n)
    assert np.array_equal(got, _single(it, d_frames, d_aligned.data_ptr(), w, h, 0.3, n))
    _hold(f"interpolate_device 1px/lane (flow pointer not 16-byte aligned) {ffmt}", got, frames[:-1], frames[1:], flow, 0.3, ((w, h), 0.3))
    got = _multi(it, d_frames, d_shifted.data_ptr() + vector_bytes, w, h, times, n)
    assert np.array_equal(got, _multi(it, d_frames, d_aligned.data_ptr(), w, h, times, n))
    _hold(f"interpolate_multi_device 1px/lane (flow pointer not 16-byte aligned) {ffmt}", got, frames[:-1], frames[1:], flow, times,
          ((w, h), tuple(times)))


@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", [(1, 37), (37, 1), (1, 1)])
def test_tiny_frames_run_exact_arithmetic_in_fma_mode(nsc, oracle_mod, w, h, ffmt):
    n = 3
    frames = _frames(n + 1, w, h)
    d_frames = put(np.ascontiguousarray(frames))
    it = _interp(nsc, ffmt)
    flow = edge_flow(n, w, h, 0.3, 50, sigma=3.0)
    flow = flow if ffmt == "f32" else flow.astype(np.float16)
    d_flow = put(flow)
    for times in TIME_SETS:
        got = _multi(it, d_frames, d_flow.data_ptr(), w, h, times, n)
        for k, t in enumerate(times):
            assert np.array_equal(got[:, k], _single(it, d_frames, d_flow.data_ptr(), w, h, t, n)), (w, h, times, k)
            for i in range(n):
                want = oracle_mod.warp_blend(frames[i], frames[i + 1], flow[i].astype(np.float32), t)
                assert np.array_equal(got[i, k], want), (w, h, ffmt, times, k, i)


@pytest.mark.parametrize("fmt,w,h", [("bgra", 64, 48), ("rgbx", 61, 7), ("bgrx", 334, 117)])
def test_input_formats_meet_the_contract_on_the_converted_frames(nsc, fmt, w, h):
    n, times = 3, TIME_SETS[1]
    frames = _frames(n + 1, w, h)
    conv = frames[..., [2, 1, 0, 3]].copy() if fmt.startswith("bgr") else frames.copy()
    if fmt.endswith("x"):
        conv[..., 3] = 255  # the alpha byte of an X format is read as opaque
    flow = edge_flow(n, w, h, 0.25, 60)
    d_frames, d_flow = put(np.ascontiguousarray(frames)), put(flow)
    got = _multi(_interp(nsc, "f32", fmt), d_frames, d_flow.data_ptr(), w, h, times, n)
    # An X format's output alpha is 255 by definition, not a blend.  (A constant channel is also the one content the contract
    # decides nothing on: the lerp of 255 and 255 lies within an ulp of an integer at every position.)
    if fmt.endswith("x"):
        assert (got[..., 3] == 255).all()
    _hold(f"interpolate_multi_device {fmt}", got, conv[:-1], conv[1:], flow, times, ((w, h), fmt), (0, 1, 2) if fmt.endswith("x") else (0, 1, 2, 3))


# ---- block vectors -------------------------------------------------------------------------------------------------------

def _vectors(w, h, bs, seed=0):
    return np.random.default_rng(9101 + seed + 131 * w + 17 * h + bs).integers(-24, 25, (-(-h // bs), -(-w // bs), 2)).astype(np.int16)


def _bm_warp(nsc, a, b, vec, bs, times, mode):
    import torch

    h, w = a.shape[:2]
    bm = nsc.BlockMatcher(block_size=bs, search_radius=24)
    da, db, dv = put(np.ascontiguousarray(a)), put(np.ascontiguousarray(b)), put(np.ascontiguousarray(vec))
    out = guarded.empty((len(times), h, w, 4), dtype=torch.uint8, device="cuda:0")
    fb = w * h * 4
    bm.warp_device(da.data_ptr(), fb, db.data_ptr(), fb, w, h, 1, dv.data_ptr(), out.data_ptr(), times=times, mode=mode, stream=_stream())
    return fetch(out)


@pytest.mark.parametrize("bs", [8, 16, 32])
@pytest.mark.parametrize("w,h,kernel", [(33, 17, "1px/lane"), (200, 72, "2px/lane"), (328, 200, "2px/lane")])
def test_block_vector_warp_rounds_nothing_at_dyadic_times_and_meets_the_contract_elsewhere(nsc, oracle_mod, w, h, kernel, bs):
    """Integer vectors and t = 1/2, k/4, k/8: every position, fraction, product and sum is exactly representable, eps of the
    positions is zero by the derivation in tests/_warp64.py and neither form rounds anything: FMA equals EXACT equals the oracle,
    byte for byte, no tolerance.  At two times that are no simple fractions the FMA form is held to the contract."""
    a, b = _frames(2, w, h)
    vec = _vectors(w, h, bs)
    flow = bmref.dense_flow(vec, w, h, bs)
    for m in (2, 4, 8):
        times = nsc.frame_times(m)
        fma = _bm_warp(nsc, a, b, vec, bs, times, "fma")
        assert np.array_equal(fma, _bm_warp(nsc, a, b, vec, bs, times, "exact")), (w, h, bs, m)
        if m == 4 or (w, h) != (328, 200):  # (the oracle and the witness of 11 frames of 328 x 200 would take seconds)
            for k, t in enumerate(times):
                assert np.array_equal(fma[k], oracle_mod.warp_blend(a, b, flow, t)), (w, h, bs, m, k)
            _hold(f"bm warp_device {kernel}", fma, a, b, flow, times, ((w, h), bs, f"x{m}"))
    # Times without a fraction of small denominator.  With integer vectors every sample of a block has the fractions of t v, and
    # where one axis sits on a texel (a zero component, a clamped sample) s = a (1 - f) + b f: at t = 0.3, f = k / 10 + 1e-7 puts
    # a tenth of those samples 1e-5 off an integer, at t = 1/3 a third, and the contract -- rightly -- leaves them undecided
    # (measured with the emulation: decided shares of 0.44 - 0.71 at t = 1/3, 0.86 - 0.95 at t = 0.3 and 0.45).
    times = _f32([0.31415927, 0.70710677])
    _hold(f"bm warp_device {kernel}", _bm_warp(nsc, a, b, vec, bs, times, "fma"), a, b, flow, times, ((w, h), bs, "t = 0.314.., 0.707.."))


def _moving(n, w, h):
    """n frames: smooth content moving right by 1.3 px a frame, on a little fixed noise."""
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    noise = _frames(1, w, h)[0] // 8
    out = np.empty((n, h, w, 4), np.uint8)
    for k in range(n):
        xs = x - 1.3 * k
        v = 112 + 45 * np.sin(xs / 3.0) * np.cos(y / 4.0) + 50 * np.sin((xs + 2 * y) / 23.0)
        out[k, ..., 0] = np.clip(v, 0, 223)
        out[k, ..., 1] = np.clip(223 - v, 0, 223)
        out[k, ..., 2] = np.clip(v * 0.5 + 40, 0, 223)
        out[k, ..., 3] = 223
        out[k] += noise
    return out


def test_block_matching_stream_frames_meet_the_contract_with_the_vectors_it_returns(nsc):
    import torch

    w, h, bs, n = 200, 72, 16, 4
    frames = np.stack([np.roll(_frames(1, w, h)[0], (2 * k, -3 * k), (0, 1)) for k in range(n)])
    frames[2] = _frames(2, w, h)[1]  # one unrelated frame: two pairs whose vectors are whatever the search found
    bm = nsc.BlockMatcher(block_size=bs, search_radius=16)
    times = nsc.frame_times(4)
    fb, K = w * h * 4, len(times)
    d_frames = put(frames)
    ws_bytes = bm.stream_workspace_size(w, h, n)
    ws = guarded.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    nbx, nby = bm.block_grid(w, h)
    vec = guarded.empty((n - 1, nby, nbx, 2), dtype=torch.int16, device="cuda:0")
    mid = guarded.empty((n - 1, K, h, w, 4), dtype=torch.uint8, device="cuda:0")
    bm.interpolate_stream_device(d_frames.data_ptr(), fb, n, w, h, ws.data_ptr(), ws_bytes, mid.data_ptr(), times=times, mode="fma",
                                 d_vectors=vec.data_ptr(), stream=_stream())
    got, v = fetch(mid), fetch(vec)
    assert np.abs(v).max() > 0
    flow = np.stack([bmref.dense_flow(v[i], w, h, bs) for i in range(n - 1)])
    _hold("bm interpolate_stream_device", got, frames[:-1], frames[1:], flow, times, ((w, h), bs))
    # a time that is no simple fraction (see the block-vector test): the vectors do not depend on it
    times = _f32([0.31415927])
    mid = guarded.empty((n - 1, 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
    bm.interpolate_stream_device(d_frames.data_ptr(), fb, n, w, h, ws.data_ptr(), ws_bytes, mid.data_ptr(), times=times, mode="fma",
                                 stream=_stream())
    _hold("bm interpolate_stream_device", fetch(mid), frames[:-1], frames[1:], flow, times, ((w, h), bs, times[0]))


def test_flow_stream_frames_meet_the_contract_with_the_flows_it_returns(nsc):
    """FlowEstimator.interpolate_device_stream, f32 hand-off: the warp kernel behind the estimator (EXACT estimator).  The witness
    takes the flows the same call stored."""
    import torch

    w, h, n, t = 160, 96, 4, 0.3
    frames = _moving(n, w, h)
    d_frames = put(frames)
    fe = nsc.FlowEstimator(levels=3, coarse_iterations=20, refine_iterations=10)
    mid = guarded.empty((n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
    flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    fe.interpolate_device_stream(d_frames.data_ptr(), n, w, h, t, mid.data_ptr(), flows.data_ptr(), _stream())
    got, flow = fetch(mid), fetch(flows)
    assert np.isfinite(flow).all() and np.abs(flow).max() > 0.25
    _hold("flow interpolate_device_stream", got, frames[:-1], frames[1:], flow, t, ((w, h), t))


def test_every_fma_warp_entry_was_held_to_the_contract():
    """Runs last: the entries seen above are exactly the ways the FMA warp is reached.  Prints the measured table (pytest -rP)."""
    assert set(_STATS) == ENTRIES, (sorted(ENTRIES - set(_STATS)), sorted(set(_STATS) - ENTRIES))
    for entry, (samples, decided, differ) in sorted(_STATS.items()):
        print(f"{entry:75s} samples {samples:9d}  decided {decided / samples:.4f}  differ from all-floor {differ / samples:.2e}")
        assert decided / samples >= MIN_DECIDED
