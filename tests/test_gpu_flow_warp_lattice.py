"""nus_flow_set_warps on the GPU, across what solve_levels() of nus_flow.cpp decides for a warped level, as solve() (a pair) and solve_batch() (a chunk) call it: the estimator
itself against its CPU float32 restatement (tests/_flow_warp64.py::estimate_f32, which tests/test_flow_warp_yardstick.py holds to the
float64 witness on the same cases) over W.LATTICE -- warps 1 .. 4, one to four levels, step counts that split into launches
unevenly, no refining or no coarse steps, two and four row blocks, more than three strips, all three LDS-tile classes, sizes below a
tile -- under every set_tiled; EXACT bit for bit, FAST within the header's bound of the CPU restatement (nus_flow_set_mode: 1e-3 px
with warps = 0; with warps the larger of 1e-3 px and four times the distance of the exact f32 result from the float64 witness on
that pair -- measured on an MI355X: 1e-3 px holds everywhere but at warps = 4 on the 4-level case, 1.01e-3, and on stream pairs 5
and 7, 2.7e-3 and 1.6e-3, where the restatement itself is 1.8e-3 and 1.3e-3 px from float64; DESIGN section 8.1 has the table).  Streams cut into chunks
(NUS_FLOW_MAX_CHUNK_PAIRS, and the product's own bound of 150 pairs), a batch whose level 0 streams while level 1 runs on tiles,
interpolate_device_stream in EXACT, with f32 and f16 flows, with and without a flow buffer, and one
handle taken through warps 0 -> 2 -> 4 -> 0.  The CPU references are computed once per module run and never written to; every
device output lives in a conftest.guarded tensor and comes down through nu_scaler_amd.transfer."""
import functools

import numpy as np
import pytest

import _flow_warp64 as W
import oracle
from _warp64 import warp_contract
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

LAM = W.LATTICE_LAMBDA
FAST_CONTRACT = 1e-3  # px: nus_flow_set_mode(NUS_FLOW_FAST), "the flow within 1e-3 px of the exact one"
FAST_CONDITIONING = 4.0  # with warps: or within this many times |exact f32 - float64| on the pair, if that is more
MIN_DECIDED = 0.9  # the decided-share floor of tests/test_gpu_warp_fma_contract.py
TABLE = (3, 50, 10)  # levels, coarse and refining steps of the stream tests at 67 x 45, 173 x 70 and 192 x 128 (FlowEstimator's defaults)
CHEAP = 40000  # cells: below it the EXACT lattice runs warps = 2 as well
ENV = ("NUS_FLOW_MAX_CHUNK_PAIRS",)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _estimator(nsc, params, warps, mode="exact", tiled=1):
    levels, coarse, refine = params
    fe = nsc.FlowEstimator(levels, coarse, refine, LAM, warps=warps)
    fe.set_mode(mode)
    fe.set_tiled(tiled)
    assert fe.warps == warps
    return fe


# ---- the CPU references: once per module run, read-only --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames(w, h, n=2):
    f = W.lattice_frames(w, h, n)
    f.setflags(write=False)
    return f


def _f32_estimate(a, b, params, warps):
    levels, coarse, refine = params
    if warps == 0:
        out = oracle.flow_estimate(a, b, levels, coarse, refine, LAM)
    else:
        out = W.estimate_f32(oracle, a, b, levels, coarse, refine, LAM, warps=warps)
    assert out.dtype == np.float32 and out.shape == a.shape[:2] + (2,)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(case, warps):
    """estimate_f32 of the case's pair.  (Without a round to run -- one level, no refining steps -- the restatement does not read
    `warps`: one array serves them all.)"""
    w, h = case[:2]
    if warps > 1 and (case[2] == 1 or case[4] == 0):
        return _reference(case, 1)
    a, b = _frames(w, h)
    return _f32_estimate(a, b, case[2:], warps)


@functools.lru_cache(maxsize=None)
def _pair_reference(w, h, params, warps, k):
    """estimate_f32 of frames (k, k + 1) of the cyclic sequence, k in 0 .. 7."""
    fr = _frames(w, h, W.LATTICE_PERIOD + 1)
    return _f32_estimate(fr[k], fr[k + 1], params, warps)


def _stream_reference(w, h, params, warps, n_pairs):
    return [_pair_reference(w, h, params, warps, k % W.LATTICE_PERIOD) for k in range(n_pairs)]


def _assert_bits(got, want, tag):
    """Equality of the float32 words; the message carries the largest |difference| and the first differing cell."""
    assert got.dtype == np.float32 and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    if diff.any():
        first = tuple(int(v) for v in np.argwhere(diff)[0])
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(got.astype(np.float64) - want)))
        raise AssertionError(f"{tag}: {int(diff.sum())} of {diff.size} floats differ from the float32 restatement, max |difference| {worst:.3g} px"
                             f"{'' if np.isfinite(got).all() else ' (not every float is finite)'}, first differing cell (.., y, x, component) "
                             f"{first}: got {float(got[first])!r}, want {float(want[first])!r}")


@functools.lru_cache(maxsize=None)
def _f32_from_f64(w, h, params, warps, k):
    """How far the exact arithmetic itself is from the float64 witness on pair k of the sequence: what the estimate makes of
    differences of a few ulps."""
    fr = _frames(w, h) if k == 0 else _frames(w, h, W.LATTICE_PERIOD + 1)
    levels, coarse, refine = params
    return float(np.abs(_f32_estimate(fr[k], fr[k + 1], params, warps) - W.estimate(fr[k], fr[k + 1], levels, coarse, refine, LAM, warps=warps)).max())


def _fast_bound(dist, w, h, params, warps, k=0):
    """The header's bound for a FAST flow at distance `dist` from the CPU restatement (the witness runs only where 1e-3 is missed)."""
    if warps == 0 or dist <= FAST_CONTRACT:
        return FAST_CONTRACT
    d64 = _f32_from_f64(w, h, params, warps, k % W.LATTICE_PERIOD)
    print(f"FAST beyond 1e-3 px | {w}x{h}, {params[0]} levels {params[1]} + {params[2]}, warps {warps}, pair {k} | {dist:.3g} px | exact f32 from float64 "
          f"{d64:.3g} px | {dist / d64:.2f}x |")
    return max(FAST_CONTRACT, FAST_CONDITIONING * d64)


def _distance(got, want, tag):
    assert got.shape == want.shape and np.isfinite(got).all(), tag
    return float(np.abs(got.astype(np.float64) - want).max())


# ---- section 2: EXACT, the estimator is the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.LATTICE, ids=W.lattice_id)
def test_exact_estimate_is_the_float32_restatement(nsc, case):
    w, h = case[:2]
    a, b = _frames(w, h)
    no_round = case[2] == 1 or case[4] == 0
    zero = {}
    if no_round:  # the bytes of a handle that never had the setting on -- and the oracle's estimator
        for tiled in (0, 1, 2, 3):
            zero[tiled] = _estimator(nsc, case[2:], 0, "exact", tiled).estimate(a, b, w, h)
            _assert_bits(zero[tiled], _reference(case, 0), (case, "warps 0", tiled))
    if case[2] == 1:
        assert np.array_equal(_reference(case, 1).view(np.uint32), oracle.flow_estimate(a, b, *case[2:], LAM).view(np.uint32))
    for warps in ((1, 2, 3, 4) if w * h <= CHEAP else (1, 3, 4)):
        want = _reference(case, warps)
        for tiled in (0, 1, 2, 3):
            got = _estimator(nsc, case[2:], warps, "exact", tiled).estimate(a, b, w, h)
            _assert_bits(got, want, (W.lattice_id(case), f"warps {warps}", f"set_tiled({tiled})"))
            if no_round:
                assert np.array_equal(got.view(np.uint32), zero[tiled].view(np.uint32)), (case, warps, tiled)
    if not no_round and w * h > 16:  # the setting is on: another round, another estimate
        assert _distance(_reference(case, 1), _reference(case, 4), case) > 0.05


@pytest.mark.parametrize("case", [c for c in W.LATTICE if c[:2] in ((130, 71), (173, 70), (64, 129), (5, 3), (333, 262))], ids=W.lattice_id)
def test_exact_estimate_device_is_the_float32_restatement(nsc, case):
    """The device entry point: the bytes of the host entry point."""
    import torch

    w, h = case[:2]
    d = put(_frames(w, h), "cuda:0")
    fb = w * h * 4
    for warps in (1, 3, 4):
        for tiled in (1, 3):
            fl = guarded.full((h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
            _estimator(nsc, case[2:], warps, "exact", tiled).estimate_device(d.data_ptr(), d.data_ptr() + fb, w, h, fl.data_ptr(), _stream())
            _assert_bits(fetch(fl), _reference(case, warps), (W.lattice_id(case), "estimate_device", f"warps {warps}", f"set_tiled({tiled})"))
    assert np.array_equal(fetch(d), _frames(w, h))


# ---- section 3: FAST, within the header's contract of the CPU restatement ---------------------------------------------------------------
@pytest.mark.parametrize("case", W.LATTICE, ids=W.lattice_id)
def test_fast_estimate_is_within_the_contract_of_the_float32_restatement(nsc, case):
    w, h = case[:2]
    a, b = _frames(w, h)
    figures = {}
    for warps in (0, 1, 4):  # (0: whether the setting is what a miss comes from)
        for tiled in (1, 2, 3):
            got = _estimator(nsc, case[2:], warps, "fast", tiled).estimate(a, b, w, h)
            figures[warps, tiled] = _distance(got, _reference(case, warps), (case, warps, tiled))
    print(f"FAST lattice | {W.lattice_id(case)} | " + " | ".join(f"{figures[wn, t]:.2e}" for wn in (0, 1, 4) for t in (1, 2, 3)) + " |")
    for (warps, tiled), d in figures.items():
        assert d <= _fast_bound(d, w, h, case[2:], warps), (W.lattice_id(case), f"warps {warps}", f"set_tiled({tiled})", d)


# ---- section 4: streams ------------------------------------------------------------------------------------------------------------------
def _run_stream(nsc, d_frames, n, w, h, params, warps, mode, tiled):
    import torch

    flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    _estimator(nsc, params, warps, mode, tiled).estimate_device_stream(d_frames.data_ptr(), n, w, h, flows.data_ptr(), _stream())
    return fetch(flows)


def _hold_stream(nsc, w, h, n, params, warps, settings, tag):
    frames = _frames(w, h, n)
    want = np.stack(_stream_reference(w, h, params, warps, n - 1))
    d = put(frames, "cuda:0")
    for mode, tiled in settings:
        got = _run_stream(nsc, d, n, w, h, params, warps, mode, tiled)
        if mode == "exact":
            _assert_bits(got, want, (tag, f"{w}x{h}", f"{n} frames", f"warps {warps}", f"set_tiled({tiled})"))
        else:
            per_pair = [_distance(got[k], want[k], (tag, k)) for k in range(n - 1)]
            print(f"FAST stream | {tag} | {w}x{h}, {n} frames, {params[0]} levels {params[1]} + {params[2]} | warps {warps} | set_tiled({tiled}) | "
                  f"{max(per_pair):.2e} | " + " ".join(f"{v:.2e}" for v in per_pair[:W.LATTICE_PERIOD]))
            for k, v in enumerate(per_pair):
                assert v <= _fast_bound(v, w, h, params, warps, k), (tag, mode, tiled, k, per_pair[:W.LATTICE_PERIOD])
    assert np.array_equal(fetch(d), frames)  # the frames are inputs


@pytest.mark.parametrize("w,h", [(67, 45), (173, 70)])
@pytest.mark.parametrize("warps", [0, 1, 4])  # (0: FAST's 1e-3 px on the same pairs without the setting)
@pytest.mark.parametrize("chunk", ["3", "1"])
def test_stream_cut_into_small_chunks(nsc, monkeypatch, w, h, warps, chunk):
    """9 frames = 8 pairs in chunks of 3, 3, 2 (and of 1): coefficient planes, flow buffers and luminance planes are indexed by the
    pair's place in its chunk, the caller's buffers by its place in the stream."""
    monkeypatch.setenv("NUS_FLOW_MAX_CHUNK_PAIRS", chunk)
    _hold_stream(nsc, w, h, 9, TABLE, warps, [("exact", 0), ("exact", 1), ("exact", 2), ("exact", 3), ("fast", 1), ("fast", 3)],
                 f"chunks of {chunk}")


def test_stream_beyond_the_chunk_bound_of_150_pairs(nsc, monkeypatch):
    """153 frames = 152 pairs = chunks of 150 + 2 with nothing overridden; pair k is reference pair k mod 8."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    _hold_stream(nsc, 67, 45, 153, TABLE, 1, [("exact", 1), ("fast", 1)], "150 + 2 pairs")


def test_stream_with_level_0_streamed_and_level_1_on_tiles(nsc, monkeypatch):
    """40 pairs of 333 x 262 in auto mode: level 0 has the 1024 waves the streamed kernel asks for, level 1 does not."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    _hold_stream(nsc, 333, 262, 41, (3, 50, 6), 1, [("exact", 1), ("fast", 1)], "mixed kernels")


def test_stream_in_the_largest_tile_class(nsc, monkeypatch):
    """4 pairs of 613 x 517: 20 x 17 x 4 = 1360 tiles of 32 x 32 in the batch."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    _hold_stream(nsc, 613, 517, 5, (2, 50, 5), 2, [("exact", 1), ("fast", 1)], "largest tile class")


# ---- section 5: the interpolating entry point --------------------------------------------------------------------------------------------
def _interpolate(nsc, d_frames, n, w, h, t, warps, mode, tiled, ffmt, with_flows):
    import torch

    fe = _estimator(nsc, TABLE, warps, mode, tiled)
    mid = guarded.empty((n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
    flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32 if ffmt == "f32" else torch.float16, device="cuda:0")
    fe.interpolate_device_stream(d_frames.data_ptr(), n, w, h, t, mid.data_ptr(), flows.data_ptr() if with_flows else 0, _stream(), ffmt)
    got_flows = fetch(flows)
    if not with_flows:  # nothing was stored there
        assert np.isnan(got_flows.astype(np.float32)).all()
    return fetch(mid), got_flows


def _hold_frames(got, frames, flow, t, tag):
    """The FMA-mode warp contract with the flows the call returned.  The scene's alpha is 255 everywhere, the one content the
    contract decides nothing on (tests/test_gpu_warp_fma_contract.py): it is held, and the floor is asked of the three channels
    that carry content."""
    st = warp_contract(got, frames[:-1], frames[1:], flow, t, 0.5, tag, channels=(0, 1, 2))
    share = st["decided"] / st["samples"]
    print(f"{tag}: samples {st['samples']}, decided {share:.4f}, differ from all-floor {st['differ_from_floor'] / st['samples']:.2e}")
    assert share >= MIN_DECIDED, (tag, share)
    warp_contract(got, frames[:-1], frames[1:], flow, t, 0.5, tag + ("alpha",), channels=(3,))


@pytest.mark.parametrize("w,h", [(173, 70), (192, 128)])
@pytest.mark.parametrize("warps", [1, 4])
@pytest.mark.parametrize("mode,tiled", [("exact", 1), ("exact", 0), ("fast", 3)])
def test_interpolate_device_stream(nsc, monkeypatch, w, h, warps, mode, tiled):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    n, t = 5, 0.3
    frames = _frames(w, h, n)
    want = np.stack(_stream_reference(w, h, TABLE, warps, n - 1))
    assert float(np.abs(want).max()) > 1.5
    d = put(frames, "cuda:0")
    for ffmt in ("f32", "f16"):
        mid, flows = _interpolate(nsc, d, n, w, h, t, warps, mode, tiled, ffmt, True)
        tag = (f"{w}x{h}", f"warps {warps}", mode, f"set_tiled({tiled})", ffmt)
        if mode == "exact" and ffmt == "f32":
            _assert_bits(flows, want, tag)
        elif mode == "exact":  # the f32 flow rounded to nearest even
            assert flows.dtype == np.float16 and np.array_equal(flows.view(np.uint16), want.astype(np.float16).view(np.uint16)), tag
        elif ffmt == "f32":
            per_pair = [_distance(flows[k], want[k], tag) for k in range(n - 1)]
            print(f"FAST stream | interpolate_device_stream | {w}x{h}, {n} frames, 3 levels 50 + 10 | warps {warps} | set_tiled({tiled}) | "
                  f"{max(per_pair):.2e} |")
            for k, v in enumerate(per_pair):
                assert v <= _fast_bound(v, w, h, TABLE, warps, k), (tag, k, per_pair)
        else:
            assert np.isfinite(flows.astype(np.float32)).all(), tag
        _hold_frames(mid, frames, flows, t, tag)
        # no flow buffer: the flows stay in the workspace (and are converted beside it); the same frames
        mid_only, _ = _interpolate(nsc, d, n, w, h, t, warps, mode, tiled, ffmt, False)
        assert np.array_equal(mid_only, mid), tag
    assert np.array_equal(fetch(d), frames)


# ---- section 6: one handle, changing warps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tiled", [("exact", 1), ("fast", 3)])
def test_one_handle_through_warps_0_2_4_0(nsc, monkeypatch, mode, tiled):
    """Raising warps on a used handle grows the coefficient planes (and a larger size every slot); lowering it leaves them too
    large.  At every stop a pair call and a 5-frame stream call give the bytes of a fresh handle created with that setting."""
    import torch

    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    n = 5
    sizes = [(67, 45), (333, 262), (67, 45)]
    dev = {size: put(_frames(*size, n), "cuda:0") for size in set(sizes)}

    def run(fe, size):
        w, h = size
        d, fb = dev[size], size[0] * size[1] * 4
        pair = guarded.full((h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
        fe.estimate_device(d.data_ptr() + fb, d.data_ptr() + 2 * fb, w, h, pair.data_ptr(), _stream())
        flows = guarded.full((n - 1, h, w, 2), float("nan"), dtype=torch.float32, device="cuda:0")
        fe.estimate_device_stream(d.data_ptr(), n, w, h, flows.data_ptr(), _stream())
        return fetch(pair), fetch(flows)

    fresh = {}
    for warps in (0, 2, 4):
        for size in set(sizes):
            fresh[warps, size] = run(_estimator(nsc, TABLE, warps, mode, tiled), size)
            assert np.isfinite(fresh[warps, size][0]).all() and np.isfinite(fresh[warps, size][1]).all()
            if mode == "exact":  # (the stream's pair 1 is the pair call's pair)
                assert np.array_equal(fresh[warps, size][0].view(np.uint32), fresh[warps, size][1][1].view(np.uint32)), (warps, size)
    assert _distance(fresh[0, (67, 45)][0], fresh[2, (67, 45)][0], "0 / 2") > 0.05
    assert _distance(fresh[2, (67, 45)][0], fresh[4, (67, 45)][0], "2 / 4") > 0.01
    used = _estimator(nsc, TABLE, 0, mode, tiled)
    for warps in (0, 2, 4, 0):
        used.set_warps(warps)
        assert used.warps == warps
        for stop, size in enumerate(sizes):
            pair, flows = run(used, size)
            assert np.array_equal(pair.view(np.uint32), fresh[warps, size][0].view(np.uint32)), (mode, warps, stop, size, "pair")
            assert np.array_equal(flows.view(np.uint32), fresh[warps, size][1].view(np.uint32)), (mode, warps, stop, size, "stream")
    if mode == "exact":  # and the fresh handles' bytes are the restatement's
        for warps in (0, 2, 4):
            _assert_bits(fresh[warps, (67, 45)][1], np.stack(_stream_reference(67, 45, TABLE, warps, n - 1)), ("fresh handle", warps))
