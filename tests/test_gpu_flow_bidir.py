"""nus_flow_set_bidirectional on the MI355X, held to flows computed on the CPU.

With the setting on the estimator's interpolating entry points solve every pair both ways and warp with the select kernel.  The
backward flow never leaves the workspace, so only the frames can show that it is wrong -- and tests/test_gpu_flow_select.py compares
them with the GPU estimator run a second time with the frames exchanged, where a defect the two uses share cancels.  Here:

  EXACT    the frames of every case of CASES are, byte for byte, nus_interp_interpolate_select_device in FMA mode fed with the
           float32 RESTATEMENT of the forward and of the backward estimate (tests/_flow_median.py::estimate_f32 of (A, B) and of
           (B, A), rounded to f16 where the hand-off is Rg16Float): test_gpu_flow_workspace.select_frames, shared with the
           workspace lattice.  tests/test_gpu_flow_select_forms.py holds that entry point to its own restatement, which closes
           the chain.  d_flows, when given, is the restated forward flow and the bytes of the same call with the setting off.
           Every set_tiled, both hand-offs, the special step counts, two to six frames, chunked streams, a cut pair, frames small
           enough for the one-pixel select kernels.
  FAST     the backward solve is by design not a FAST estimate of (B, A): what is exact is held exactly (d_flows, repeats, a fresh
           handle, a poisoned workspace), and every pixel to the warp contract with either candidate taken from the EXACT
           restatement, widened by FAST's stated flow bound.
  cost     off after on is a fresh handle (tests/test_gpu_flow_select.py); on, the workspace grows by at most 28 B per pixel and pair.

Every device output comes from conftest.guarded; CPU references are computed once (the workspace module's caches)."""
import numpy as np
import pytest

import _flow_select as S
import test_gpu_flow_workspace as WS
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

C, IDS, IMS = WS.C, WS.IDS, WS.IMS
S97, S64, S33, S160 = WS.S97, WS.S64, WS.S33, WS.S160
FMA_POSITION_ULPS = 0.5  # the warp behind the estimator runs in FMA mode (tests/test_gpu_warp_fma_contract.py)
FAST_FLOW_BOUND = 1e-3  # px: nus_flow_set_mode(NUS_FLOW_FAST) at warps 0 (include/nuscaler_hip.h)


def B(entry, size, steps=(3, 9, 6), tiled=1, **kw):
    return C(entry, size, steps, tiled, bidir=True, **kw)


# Sparse, as the workspace lattice's: every entry x set_tiled, every setting's values on the batch and on the pair-by-pair road,
# every special step count on both, 2, 4 and 6 frames, the four sizes (97 x 61: odd on every level).
CASES = [
    B(IDS, S97, (3, 9, 6), 0, n=4, ffmt="f32", flows=True),
    B(IDS, S160, (4, 11, 3), 0, project=2, n=4, ffmt="f16", flows=False),
    B(IDS, S97, (3, 0, 6), 0, warps=2, median=5, n=2, ffmt="f16", flows=True),  # no coarse steps: the cleared flow
    B(IMS, S160, (1, 9, 6), 0, median=3, n=2, ffmt="f32", flows=True),  # one level
    B(IMS, S64, (3, 9, 0), 0, warps=2, project=2, n=6, ffmt="f32", flows=False),  # no refining steps: upsamples only
    B(IMS, S97, (4, 11, 3), 1, warps=2, median=3, project=2, n=4, ffmt="f16", flows=False),  # two launches a level, four levels
    B(IDS, S160, (1, 0, 6), 1, project=2, n=4, ffmt="f16", flows=True),  # one level and no step at all: both flows are the cleared one
    B(IMS, S64, (3, 9, 0), 1, median=5, n=6, ffmt="f32", flows=True),
    B(IDS, S33, (3, 9, 6), 1, warps=2, n=2, ffmt="f32", flows=False),
    B(IDS, S64, (3, 0, 6), 2, median=5, n=2, ffmt="f16", flows=True),
    B(IMS, S97, (1, 9, 6), 2, n=4, ffmt="f16", flows=False),
    B(IMS, S160, (3, 9, 6), 2, warps=2, project=2, n=4, ffmt="f32", flows=True),
    B(IMS, S33, (3, 9, 0), 3, warps=2, project=2, n=6, ffmt="f32", flows=False),
    B(IDS, S97, (4, 11, 3), 3, warps=2, median=3, n=4, ffmt="f32", flows=True),
    B(IMS, S64, (1, 0, 6), 3, median=3, n=2, ffmt="f16", flows=True),
    B(IDS, S160, (3, 9, 6), 3, median=5, project=2, n=6, ffmt="f16", flows=False),
    # ---- chunks of 2, 2 and 1 pairs: J.pairs(c0, n) advances the frames, mid, d_flows and the first pair together, and every chunk
    # reuses the three slots of the setting
    B(IDS, S97, (3, 9, 6), 1, warps=2, median=3, n=6, ffmt="f32", flows=True, chunk=2),
    B(IMS, S160, (3, 9, 6), 3, project=2, n=6, ffmt="f16", flows=False, chunk=2),
    B(IMS, S97, (3, 9, 6), 2, n=6, ffmt="f16", flows=True, chunk=2),
    # ---- scene detection behind the warp: pair 2 is a cut
    B(IMS, S160, (3, 9, 6), 1, warps=2, project=2, n=5, ffmt="f32", flows=True, scene=True),
    B(IMS, S160, (3, 9, 6), 0, median=3, n=5, ffmt="f16", flows=False, scene=True),
]
assert len(set(CASES)) == len(CASES)


def _env(monkeypatch, c):
    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    if c.chunk:
        monkeypatch.setenv(WS.CHUNK_ENV, str(c.chunk))
    else:
        monkeypatch.delenv(WS.CHUNK_ENV, raising=False)


@pytest.mark.parametrize("c", CASES, ids=WS.case_id)
def test_exact_frames_are_the_select_warp_of_the_cpu_flows(nsc, monkeypatch, c):
    _env(monkeypatch, c)
    tag = WS.case_id(c)
    d = put(WS._frames(c.size, c.n, c.scene), "cuda:0")
    on = WS._call(WS._estimator(nsc, c), c, d)
    WS._assert_restated(c, on, nsc)  # the frames: select_frames; d_flows, when given: the restated forward flows
    off_case = c._replace(bidir=False)
    off = WS._call(WS._estimator(nsc, off_case), off_case, d)
    if c.flows:  # d_flows: the forward flows only, the bytes of the setting off
        assert np.array_equal(on["flows"].view(np.uint8), off["flows"].view(np.uint8)), (tag, "d_flows differs from the setting off")
    fwd = np.stack([WS._restated(c.size, c.n, c.scene, c.steps, c.warps, c.median, k) for k in range(c.n - 1)])
    bwd = np.stack([WS._restated(c.size, c.n, c.scene, c.steps, c.warps, c.median, k, True) for k in range(c.n - 1)])
    if c.steps[1:] != (0, 6) or c.steps[0] > 1:  # (one level and no step: both flows are zero, and the frames the plain blend's)
        assert float(np.abs(fwd).max()) > 1.0 and float(np.abs(fwd + bwd).max()) > 0.25, tag  # motion, and no mirror images
        assert not np.array_equal(on["mid"], off["mid"]), (tag, "the setting does nothing here")
    else:
        assert not fwd.any() and not bwd.any() and np.array_equal(on["mid"], off["mid"]), tag
    if c.chunk:  # EXACT: the chunked stream's frames are the unchunked one's
        monkeypatch.delenv(WS.CHUNK_ENV)
        WS._assert_same_bytes(WS._call(WS._estimator(nsc, c), c, d), on, (tag, "chunked against unchunked"))
    if c.scene:
        WS._assert_cut_pair(c, on)
    assert np.array_equal(fetch(d), WS._frames(c.size, c.n, c.scene)), tag  # the frames are inputs


# frames of 2 x 2 (the smallest the tile kernel takes) and below it: k_warp_blend_flow_sel_tiny behind the estimator.  One level;
# below 2 x 2 on the pair-by-pair road, whose kernels are the host primitives' (held at 1 x 1 by tests/test_flow.py).
@pytest.mark.parametrize("c", [B(IMS, (2, 2), (1, 9, 6), 0, n=3, ffmt="f32", flows=True), B(IDS, (2, 2), (1, 9, 6), 1, n=3, ffmt="f16", flows=False),
                               B(IMS, (1, 1), (1, 9, 6), 0, n=3, ffmt="f16", flows=True), B(IDS, (1, 1), (1, 9, 6), 0, n=3, ffmt="f32", flows=False),
                               B(IMS, (5, 1), (1, 9, 6), 0, project=2, n=3, ffmt="f32", flows=False),
                               B(IDS, (5, 1), (1, 9, 6), 0, median=3, n=3, ffmt="f16", flows=True)], ids=WS.case_id)
def test_smallest_frames(nsc, monkeypatch, c):
    _env(monkeypatch, c)
    d = put(WS._frames(c.size, c.n), "cuda:0")
    fe = WS._estimator(nsc, c)
    on = WS._call(fe, c, d)
    WS._assert_restated(c, on, nsc)
    fe._fill_workspace(0xFF, WS._stream())
    WS._assert_same_bytes(WS._call(fe, c, d), on, (WS.case_id(c), "after a fill with 0xff"))


@pytest.mark.parametrize("tiled", [0, 1, 3])
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
def test_single_time_frame_is_the_multi_time_frame_at_that_time(nsc, monkeypatch, ffmt, tiled):
    """nus_flow_interpolate_device_stream at t = times[j] is frame j of nus_flow_interpolate_multi_device_stream, on one handle."""
    import torch

    monkeypatch.delenv(WS.CHUNK_ENV, raising=False)
    c = B(IMS, S97, (3, 9, 6), tiled, warps=2, median=3, project=2, n=4, ffmt=ffmt, flows=False)
    w, h = c.size
    d = put(WS._frames(c.size, c.n), "cuda:0")
    fe = WS._estimator(nsc, c)
    multi = WS._call(fe, c, d)["mid"]
    WS.assert_select_frames(nsc, c, {"mid": multi})
    for j, t in enumerate(WS.TIMES):
        one = guarded.empty((c.n - 1, h, w, 4), dtype=torch.uint8, device="cuda:0")
        fe.interpolate_device_stream(d.data_ptr(), c.n, w, h, t, one.data_ptr(), 0, WS._stream(), ffmt)
        assert np.array_equal(fetch(one), multi[:, j]), (ffmt, tiled, t)


# ---- FAST -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("tiled", [1, 3])
def test_fast_frames_meet_the_warp_contract_with_a_restated_candidate(nsc, monkeypatch, tiled, ffmt):
    """FAST with the setting on.  (fast, 3) is the case the setting's own description singles out: the forward solve runs
    k_hs_stream_fast and the backward solve the exact kernels on coefficient planes built from the FAST pyramid -- by design not
    the bytes of a FAST estimate of (B, A), so there is no byte reference for the frames.

    Exact first: d_flows is the setting-off bytes; a repeat, a fresh handle and a handle whose workspace was poisoned give the
    same bytes.  Then the contract: every pixel meets tests/_flow_select.py::contract_pixels with gF or gR taken from the EXACT
    restated flows, the position band widened by the bound the header states for FAST at warps 0, 1e-3 px per component (for the
    Rg16Float hand-off plus half an f16 ulp of the largest component, 2^-9 px below 8 px: the halves are a rounding of the FAST
    flow, not of the restated one).  That band admits either neighbouring count of a sample almost everywhere, so this is a
    plus-or-minus-one-count check: it catches a wrong plane, pair or direction, not a rounding.  The sharp checks of the backward
    solve are the EXACT ones above."""
    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    monkeypatch.delenv(WS.CHUNK_ENV, raising=False)
    c = B(IMS, S160, (3, 9, 6), tiled, mode="fast", n=4, ffmt=ffmt, flows=True)
    tag = WS.case_id(c)
    frames = WS._frames(c.size, c.n)
    d = put(frames, "cuda:0")
    fe = WS._estimator(nsc, c)
    first = WS._call(fe, c, d)
    off_case = c._replace(bidir=False)
    off = WS._call(WS._estimator(nsc, off_case), off_case, d)
    assert np.array_equal(first["flows"].view(np.uint8), off["flows"].view(np.uint8)), (tag, "d_flows differs from the setting off")
    assert not np.array_equal(first["mid"], off["mid"]), (tag, "the setting does nothing here")
    WS._assert_same_bytes(WS._call(fe, c, d), first, (tag, "a repeat"))
    WS._assert_same_bytes(WS._call(WS._estimator(nsc, c), c, d), first, (tag, "a fresh handle"))
    fe._fill_workspace(0xFF, WS._stream())
    WS._assert_same_bytes(WS._call(fe, c, d), first, (tag, "after a fill with 0xff"))
    exact = c._replace(mode="exact")
    fwd = np.stack([WS._restated(c.size, c.n, False, c.steps, 0, 0, k) for k in range(c.n - 1)])
    bwd = np.stack([WS._restated(c.size, c.n, False, c.steps, 0, 0, k, True) for k in range(c.n - 1)])
    assert float(max(np.abs(fwd).max(), np.abs(bwd).max())) < 8.0
    band = FAST_FLOW_BOUND + (2.0 ** -9 if ffmt == "f16" else 0.0)
    apart = float(np.abs(first["flows"].astype(np.float64) - fwd).max())
    print(f"{tag}: d_flows within {apart:.3g} px of the EXACT restatement (band {band:.3g})")
    assert apart <= band, (tag, apart)  # FAST's own contract, on the flow that can be seen
    exact_frames = WS.select_frames(nsc, exact)
    near = float((first["mid"] == exact_frames).mean())
    print(f"{tag}: {near:.4f} of the bytes are the EXACT handle's")
    only = {"forward": 0, "backward": 0}
    for k in range(c.n - 1):
        for j, t in enumerate(WS.TIMES):
            ok_f = S.contract_pixels(first["mid"][k, j], frames[k], frames[k + 1], fwd[k], t, FMA_POSITION_ULPS, band)
            ok_r = S.contract_pixels(first["mid"][k, j], frames[k], frames[k + 1], -bwd[k], t, FMA_POSITION_ULPS, band)
            bad = ~(ok_f | ok_r)
            assert not bad.any(), (tag, k, t, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            only["forward"] += int((ok_f & ~ok_r).sum())
            only["backward"] += int((ok_r & ~ok_f).sum())
    print(f"{tag}: pixels only the forward candidate explains {only['forward']}, only the backward one {only['backward']}")
    assert only["forward"] > 0 and only["backward"] > 0, (tag, only)  # both candidates are in use, and the check tells them apart


# ---- what the setting costs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [B(IMS, S160, tiled=1, n=4, ffmt="f32", flows=False), B(IMS, S160, tiled=1, n=4, ffmt="f32", flows=True),
                               B(IDS, S97, tiled=3, warps=2, n=5, ffmt="f16", flows=False), B(IDS, S97, tiled=2, median=3, n=5, ffmt="f16", flows=True),
                               B(IMS, S160, tiled=0, n=4, ffmt="f16", flows=False), B(IDS, S160, tiled=0, n=4, ffmt="f32", flows=True),
                               B(IMS, S160, tiled=3, mode="fast", n=4, ffmt="f16", flows=False),
                               B(IDS, S97, tiled=1, n=6, ffmt="f32", flows=False, chunk=2)], ids=WS.case_id)
def test_the_setting_adds_at_most_28_bytes_per_pixel_and_pair(nsc, monkeypatch, c):
    """include/nuscaler_hip.h: 28 B per pixel and pair more -- two flow buffers (the forward flows kept from the backward solve
    and the backward flows, 8 B each) and the backward solve's coefficients (12 B), for the pairs of the largest chunk (the
    pair-by-pair road holds one pair's).  DeviceBuffer::reserve allocates exactly the bytes it is asked for, so the three slots
    add no rounding: the bound is the product itself."""
    import torch

    _env(monkeypatch, c)
    d = put(WS._frames(c.size, c.n), "cuda:0")
    held = {}
    for on in (False, True):
        case = c._replace(bidir=on)
        fe = WS._estimator(nsc, case)
        WS._call(fe, case, d)
        torch.cuda.synchronize()
        held[on] = fe.workspace_bytes
    chunk_pairs = 1 if WS.path_of(c).startswith(WS.PER_STEP) else min(c.n - 1, c.chunk or c.n - 1)
    bound = 28 * c.size[0] * c.size[1] * chunk_pairs
    print(f"{WS.case_id(c)}: off {held[False]} B, on {held[True]} B: {held[True] - held[False]} B more, bound {bound} B")
    assert 0 < held[True] - held[False] <= bound, (WS.case_id(c), held, bound)
