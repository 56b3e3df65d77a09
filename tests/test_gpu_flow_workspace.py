"""No result of a nus_flow handle depends on what its device workspace held before the call.

The estimator keeps twelve grow-only slots that come straight from hipMalloc and are never cleared; four of them carry two names
(the pair path's kImage / kTemp / kPyrA / kPyrB are the batch path's kLevelInOdd / kLevelInEven / kLum / kCoef), the coarsest level
starts from a null flow pointer instead of a cleared buffer, the fast pyramid writes one float per pixel into buffers sized for
four, tiles, strips and medians load halos and ragged last rows and mask them afterwards, row blocks and chunks reuse the same
planes.  A kernel that reads a cell nobody wrote, or a schedule that forgets a clear, passes every other test of the suite as long
as the stale cell holds zero or the flow of the same scene.  Here the workspace is poisoned from inside (TEST HOOK
nus_flow_fill_workspace, FlowEstimator._fill_workspace) between identical calls:

* the lattice: CASES, one table.  Per case, on one handle: the call once (the workspace reaches its size), then per fill byte of
  BYTES the fill and the identical call into fresh conftest.guarded outputs.  workspace_bytes never moves again, every output of
  every repeat is byte-equal to the first call's and to a fresh handle's, a flow buffer that was not given keeps its NaN fill, and
  the EXACT flows equal the float32 restatement of the estimator (tests/_flow_median.py::estimate_f32, which is
  oracle.flow_estimate at warps = median = 0 and _flow_warp64's estimator at median = 0); the primitives equal theirs.  FAST cases
  are held to byte equality as well: the same kernels on the same inputs.
  nus_flow_set_bidirectional adds three slots of its own (the forward flows kept from the backward solve, the backward flows, the
  backward solve's coefficients) and a flow that never leaves the workspace: cases with the setting on are held in the same way,
  and their EXACT frames to the select warp of the CPU-restated forward and backward flows (select_frames, shared with
  tests/test_gpu_flow_bidir.py).
* history without poison, across the slot aliases: A, B, A on one handle (HISTORY), the setting on, off and on again among them.
* the stream rule of the header: two calls of different shape and content back to back on ONE stream with no host
  synchronisation between them, primed, primed and poisoned, and with the second call growing the workspace.

The last test holds the census: every entry x set_tiled x mode, every setting on every path, the special step counts and the
chunked streams were seen.  CPU references are computed once per module run and never written to; device outputs come down
through nu_scaler_amd.transfer."""
import collections
import functools

import numpy as np
import pytest

import _flow_median as M
import _flow_project as PJ
import _flow_warp64 as W
import _scenecut as sc
import oracle
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

LAM = 0.02 ** 2  # FlowEstimator's default
# what a fill byte makes of a cell, and what it exposes:
#   0x00  zero                                                    the baseline
#   0xFF  NaN in every f32 and f16 cell, 255 in every flag        reads that propagate NaN (min / max / med3 swallow it)
#   0x7F  3.39e38 in f32, NaN in f16                              reads a NaN-swallowing operation hides (a clamp hides this one)
#   0x3E  0.186 in f32, 1.56 in f16                               an ordinary value: passes clamps, medians and selects alike
BYTES = (0x00, 0xFF, 0x7F, 0x3E)
TIMES = (0.25, 0.5, 0.75)  # of the multi-time entry
T_ONE = 0.3  # of the single-time entry
CHUNK_ENV = "NUS_FLOW_MAX_CHUNK_PAIRS"

S97, S64, S33, S160 = (97, 61), (64, 48), (33, 17), (160, 96)  # 97 x 61: odd sides on every level, 49 x 31, 25 x 16, 13 x 8
PAIR, BATCH, PER_STEP = "pair", "batch", "per-step"
BACKWARD = "+backward"
ESTIMATORS = ("estimate", "estimate_device", "estimate_device_stream", "interpolate_device_stream", "interpolate_multi_device_stream")
PRIMITIVES = ("rgba8_to_f32", "blur", "downsample", "horn_schunck", "horn_schunck+flow_in", "horn_schunck_coef", "horn_schunck_coef+flow_in",
              "warp_coefficients", "warp_coefficients+flow", "upsample", "median3", "median5", "project_flow")

Case = collections.namedtuple("Case", "entry size steps tiled mode warps median project n ffmt flows chunk scene bidir")


def C(entry, size, steps=(3, 9, 6), tiled=1, mode="exact", warps=0, median=0, project=0, n=2, ffmt="f32", flows=True, chunk=None,
      scene=False, bidir=False):
    """bidir: nus_flow_set_bidirectional -- both flows of every pair and the select warp behind the interpolating entry points."""
    assert not bidir or entry in ESTIMATORS[3:]  # (the estimate entry points are not affected by the setting)
    return Case(entry, size, steps, tiled, mode, warps, median, project, n, ffmt, flows, chunk, scene, bidir)


def case_id(c):
    s = f"{c.entry}-{c.size[0]}x{c.size[1]}-L{c.steps[0]}-{c.steps[1]}+{c.steps[2]}-tiled{c.tiled}-{c.mode}-w{c.warps}m{c.median}p{c.project}"
    if c.entry in ESTIMATORS[2:]:
        s += f"-{c.n}fr"
    if c.entry in ESTIMATORS[3:]:
        s += f"-{c.ffmt}-{'flows' if c.flows else 'noflows'}"
    return s + (f"-chunk{c.chunk}" if c.chunk else "") + ("-scene" if c.scene else "") + ("-bidir" if c.bidir else "")


def path_of(c):
    """Which road through nus_flow.cpp an estimator case takes: solve() for a pair, solve_batch() for a chunk (a FAST pair whose
    streamed kernel is forced goes there as a two-frame stream), or one launch per Jacobi step (set_tiled(0), EXACT).  With the
    setting on the backward solve takes the same road a second time (BACKWARD behind the name): solve() with the pyramids
    exchanged pair by pair, or solve_batch()'s second schedule on coefficient planes."""
    if c.tiled == 0 and c.mode == "exact":
        return PER_STEP + BACKWARD * c.bidir
    if c.entry in ("estimate", "estimate_device") and not (c.mode == "fast" and c.tiled == 3):
        return PAIR
    return BATCH + BACKWARD * c.bidir


IDS, IMS = "interpolate_device_stream", "interpolate_multi_device_stream"
CASES = [
    # ---- the host pair entry point
    C("estimate", S97, (3, 9, 6), 0),
    C("estimate", S97, (4, 11, 3), 1, warps=2, median=3, project=2),
    C("estimate", S64, (3, 9, 6), 2, median=5),
    C("estimate", S33, (2, 9, 6), 3, warps=2),
    C("estimate", S97, (3, 9, 6), 1, "fast"),
    C("estimate", S97, (3, 11, 3), 3, "fast", warps=2, median=5),
    # ---- the device pair entry point
    C("estimate_device", S97, (3, 9, 6), 0, warps=2, median=5, project=2),
    C("estimate_device", S97, (4, 9, 6), 1),
    C("estimate_device", S64, (3, 0, 6), 2, warps=2, median=3),  # no coarse steps: the cleared flow
    C("estimate_device", S97, (3, 9, 0), 3, median=5),  # no refining steps: upsamples only
    C("estimate_device", S97, (1, 9, 6), 1),  # one level
    C("estimate_device", S33, (2, 9, 6), 1, "fast", warps=2, median=3),
    C("estimate_device", S97, (3, 9, 6), 3, "fast"),
    # ---- streams of flows
    C("estimate_device_stream", S97, (3, 9, 6), 0, median=3, n=5),
    C("estimate_device_stream", S97, (4, 11, 3), 1, warps=2, median=5, n=5),
    C("estimate_device_stream", S64, (3, 9, 6), 2, n=4),
    C("estimate_device_stream", S97, (3, 9, 6), 3, warps=2, median=3, n=6),
    C("estimate_device_stream", S97, (3, 9, 6), 1, "fast", n=5),
    C("estimate_device_stream", S97, (4, 11, 3), 3, "fast", warps=2, n=5),
    C("estimate_device_stream", S33, (2, 0, 6), 1, n=4),
    C("estimate_device_stream", S64, (3, 0, 6), 0, n=4),
    C("estimate_device_stream", S97, (3, 9, 0), 0, warps=2, n=4),
    C("estimate_device_stream", S97, (3, 9, 0), 1, warps=2, median=3, n=4),
    C("estimate_device_stream", S97, (1, 9, 6), 3, n=4),
    C("estimate_device_stream", S97, (1, 0, 6), 1, n=4),  # one level and no step at all: the cleared flow is the result
    C("estimate_device_stream", S97, (3, 9, 6), 2, median=5, n=6, chunk=2),
    # ---- the in-between frames at one time: f32 and f16 flows, with and without a flow buffer
    C(IDS, S160, tiled=0, project=2, n=4, ffmt="f32", flows=True),
    C(IDS, S160, tiled=0, warps=2, median=3, n=4, ffmt="f16", flows=False),
    C(IDS, S160, tiled=1, warps=2, project=2, n=4, ffmt="f32", flows=False),
    C(IDS, S160, tiled=1, median=5, n=4, ffmt="f16", flows=True),
    C(IDS, S160, tiled=2, median=3, project=2, n=4, ffmt="f32", flows=True),
    C(IDS, S160, tiled=2, warps=2, n=4, ffmt="f16", flows=False),
    C(IDS, S160, tiled=3, project=2, n=4, ffmt="f16", flows=True),
    C(IDS, S160, tiled=3, warps=2, median=5, n=4, ffmt="f32", flows=False),
    C(IDS, S160, tiled=1, mode="fast", n=4, ffmt="f32", flows=True),
    C(IDS, S160, tiled=1, mode="fast", warps=2, median=3, project=2, n=4, ffmt="f16", flows=False),
    C(IDS, S160, tiled=3, mode="fast", project=2, n=4, ffmt="f16", flows=True),  # k_hs_stream_fast stores the halves itself
    C(IDS, S160, tiled=3, mode="fast", n=4, ffmt="f16", flows=False),  # ... beside the flows
    C(IDS, S160, tiled=3, mode="fast", warps=2, median=5, n=4, ffmt="f32", flows=False),
    # ---- ... in chunks of 2, 2 and 1 pairs
    C(IDS, S160, tiled=1, warps=2, median=3, n=6, ffmt="f32", flows=True, chunk=2),
    C(IDS, S160, tiled=3, n=6, ffmt="f32", flows=False, chunk=2),
    C(IDS, S160, tiled=1, mode="fast", n=6, ffmt="f16", flows=True, chunk=2),
    C(IDS, S160, tiled=3, mode="fast", warps=2, n=6, ffmt="f16", flows=False, chunk=2),
    # ---- the in-between frames at three times
    C(IMS, S160, tiled=0, n=4, ffmt="f32", flows=True),
    C(IMS, S160, tiled=1, warps=2, median=3, project=2, n=5, ffmt="f32", flows=False, scene=True),  # pair 2 is a cut
    C(IMS, S160, tiled=2, project=2, n=4, ffmt="f16", flows=True),
    C(IMS, S160, tiled=3, warps=2, median=5, n=4, ffmt="f16", flows=False),
    C(IMS, S160, tiled=1, mode="fast", n=4, ffmt="f32", flows=True),
    C(IMS, S160, tiled=3, mode="fast", warps=2, project=2, n=4, ffmt="f16", flows=False),
    # ---- both flows of every pair and the select warp behind them (nus_flow_set_bidirectional): kFwdFlows, kBwdFlows, kBwdCoef
    C(IDS, S160, tiled=0, n=4, ffmt="f32", flows=True, bidir=True),  # pair by pair: kBwdFlows holds one pair's f32 flow
    C(IDS, S160, tiled=0, warps=2, median=3, project=2, n=4, ffmt="f16", flows=False, bidir=True),  # ... and its halves behind it
    C(IDS, S160, tiled=1, warps=2, median=5, n=4, ffmt="f16", flows=True, bidir=True),
    C(IDS, S160, tiled=2, project=2, n=4, ffmt="f32", flows=False, bidir=True),  # no d_flows: the forward flows wait in kFwdFlows
    C(IDS, S160, tiled=3, median=3, n=4, ffmt="f16", flows=False, bidir=True),
    C(IDS, S160, tiled=1, mode="fast", n=4, ffmt="f32", flows=False, bidir=True),
    C(IDS, S160, tiled=3, mode="fast", warps=2, project=2, n=4, ffmt="f16", flows=True, bidir=True),  # forward: k_hs_stream_fast's halves
    C(IDS, S160, tiled=3, warps=2, n=6, ffmt="f32", flows=True, bidir=True, chunk=2),  # chunks of 2, 2 and 1 pairs
    C(IMS, S160, tiled=0, median=5, n=4, ffmt="f32", flows=False, bidir=True),
    C(IMS, S160, tiled=1, project=2, n=4, ffmt="f32", flows=True, bidir=True),
    C(IMS, S160, tiled=2, warps=2, median=3, n=4, ffmt="f16", flows=True, bidir=True),
    C(IMS, S160, tiled=3, warps=2, median=5, project=2, n=4, ffmt="f32", flows=True, bidir=True),
    C(IMS, S160, tiled=1, mode="fast", warps=2, median=3, n=4, ffmt="f16", flows=False, bidir=True),
    C(IMS, S160, tiled=3, mode="fast", n=4, ffmt="f32", flows=True, bidir=True),
    C(IMS, S160, tiled=1, warps=2, median=3, project=2, n=5, ffmt="f16", flows=False, scene=True, bidir=True),  # pair 2 is a cut
    # ---- the host primitives (steps[1]: Jacobi steps)
    C("rgba8_to_f32", S97),
    C("blur", S97),
    C("downsample", S97),
    C("horn_schunck", S97, tiled=1),
    C("horn_schunck+flow_in", S97, tiled=1),
    C("horn_schunck", S97, tiled=0),
    C("horn_schunck+flow_in", S97, tiled=3),
    C("horn_schunck", S64, tiled=2),
    C("horn_schunck_coef", S97, tiled=1),
    C("horn_schunck_coef+flow_in", S97, tiled=3),
    C("horn_schunck_coef+flow_in", S64, tiled=2),
    C("warp_coefficients", S97),
    C("warp_coefficients+flow", S97),
    C("upsample", S97),
    C("median3", S97),
    C("median5", S97),
    C("project_flow", S97),
]
assert len(set(CASES)) == len(CASES)

_SEEN = set()  # what the lattice held, for the census


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _estimator(nsc, c):
    fe = nsc.FlowEstimator(c.steps[0], c.steps[1], c.steps[2], LAM, warps=c.warps, median=c.median, project=c.project, bidirectional=c.bidir)
    assert fe.bidirectional is c.bidir
    fe.set_mode(c.mode)
    fe.set_tiled(c.tiled)
    if c.scene:
        fe.set_scene_detect(True)
    assert (fe.warps, fe.median_size, fe.project, fe.mode, fe.workspace_bytes) == (c.warps, c.median, c.project, c.mode, 0)
    return fe


# ---- inputs and CPU references: once per module run, read-only --------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _frames(size, n, scene=False):
    """n RGBA8 frames of the lattice's moving scene (pan (-2, 1), square (6, 4) px per frame); below its smallest size a crop
    around the square's edge.  scene: from frame 3 on another shot (the frames darkened to a quarter), so pair (2, 3) is a cut."""
    w, h = size
    if w >= 60 and h >= 30:
        f = W.lattice_frames(w, h, n)
    else:
        f = np.ascontiguousarray(W.lattice_frames(97, 61, n)[:, 10:10 + h, 12:12 + w])
    if scene:
        f = f.copy()
        f[3:, ..., :3] //= 4
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def _restated(size, n, scene, steps, warps, median, k, back=False):
    """The float32 restatement of the estimate of frames (k, k + 1); back: of (k + 1, k), the flow B -> A on B's grid -- the same
    schedule on the same per-frame pyramids with the two exchanged, which is what nus_flow_set_bidirectional states."""
    f = _frames(size, n, scene)
    a, b = (f[k + 1], f[k]) if back else (f[k], f[k + 1])
    out = M.estimate_f32(oracle, a, b, steps[0], steps[1], steps[2], LAM, warps=warps, median=median)
    assert out.dtype == np.float32 and out.shape == (size[1], size[0], 2)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def _primitive_inputs(size):
    w, h = size
    rng = np.random.default_rng(1000 * w + h)
    d = {"rgba8": rng.integers(0, 256, (h, w, 4), dtype=np.uint8),
         "i1": rng.random((h, w, 4), np.float32), "i2": rng.random((h, w, 4), np.float32),
         "flow": ((rng.random((h, w, 2)) - 0.5) * 6).astype(np.float32),  # +-3 px
         "small": ((rng.random(((h + 1) // 2, (w + 1) // 2, 2)) - 0.5) * 6).astype(np.float32)}
    d["coef"] = W.coefficients_f32(d["i1"], d["i2"], None)
    return {k: _frozen(v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _primitive_reference(entry, size, iterations):
    p = _primitive_inputs(size)
    w, h = size
    start = p["flow"] if entry.endswith("+flow_in") or entry.endswith("+flow") else None
    name = entry.split("+")[0]
    if name == "rgba8_to_f32":
        out = oracle.rgba8_to_f32(p["rgba8"])
    elif name == "blur":
        out = oracle.blur(p["i1"])
    elif name == "downsample":
        out = oracle.downsample(p["i1"])
    elif name == "horn_schunck":
        out = oracle.horn_schunck(p["i1"], p["i2"], start, iterations=iterations, lam=LAM)
    elif name == "horn_schunck_coef":
        out = W.jacobi_coef_f32(p["coef"], start, iterations, LAM)
    elif name == "warp_coefficients":
        out = W.coefficients_f32(p["i1"], p["i2"], start)
    elif name == "upsample":
        out = oracle.flow_upsample(p["small"], w, h, 2.0)
    elif name in ("median3", "median5"):
        out = M.median_filter(p["flow"], int(name[-1]))
    else:
        assert name == "project_flow"
        out = PJ.project_f32(p["flow"], 0.5, 2)
    return _frozen(np.asarray(out))


# ---- one call of a case -----------------------------------------------------------------------------------------------------------
def _call(fe, c, d_frames):
    """The case's call on `fe`, every device output into fresh guarded tensors -> {name: array}."""
    import torch

    w, h = c.size
    dev = "cuda:0"
    if c.entry in PRIMITIVES:
        p = _primitive_inputs(c.size)
        start = p["flow"] if "+" in c.entry else None
        name = c.entry.split("+")[0]
        if name in ("rgba8_to_f32", "blur", "downsample"):
            return {"out": getattr(fe, name)(p["rgba8"] if name == "rgba8_to_f32" else p["i1"])}
        if name == "horn_schunck":
            return {"out": fe.horn_schunck(p["i1"], p["i2"], start, c.steps[1], LAM)}
        if name == "horn_schunck_coef":
            return {"out": fe.horn_schunck_coef(p["coef"], start, c.steps[1], LAM)}
        if name == "warp_coefficients":
            return {"out": fe.warp_coefficients(p["i1"], p["i2"], start)}
        if name == "upsample":
            return {"out": fe.upsample(p["small"], w, h, 2.0)}
        if name in ("median3", "median5"):
            return {"out": fe.median(p["flow"], int(name[-1]))}
        return {"out": fe.project_flow(p["flow"], 0.5, 2)}
    frames = _frames(c.size, c.n, c.scene)
    fb = w * h * 4
    if c.entry == "estimate":
        return {"flows": fe.estimate(frames[0], frames[1], w, h)[None]}
    if c.entry == "estimate_device":
        fl = guarded.full((1, h, w, 2), float("nan"), dtype=torch.float32, device=dev)
        fe.estimate_device(d_frames.data_ptr(), d_frames.data_ptr() + fb, w, h, fl.data_ptr(), _stream())
        return {"flows": fetch(fl)}
    fdt = torch.float32 if c.ffmt == "f32" else torch.float16
    fl = guarded.full((c.n - 1, h, w, 2), float("nan"), dtype=fdt, device=dev)
    if c.entry == "estimate_device_stream":
        fe.estimate_device_stream(d_frames.data_ptr(), c.n, w, h, fl.data_ptr(), _stream())
        return {"flows": fetch(fl)}
    if c.entry == IDS:
        mid = guarded.empty((c.n - 1, h, w, 4), dtype=torch.uint8, device=dev)
        fe.interpolate_device_stream(d_frames.data_ptr(), c.n, w, h, T_ONE, mid.data_ptr(), fl.data_ptr() if c.flows else 0, _stream(), c.ffmt)
    else:
        assert c.entry == IMS
        mid = guarded.empty((c.n - 1, len(TIMES), h, w, 4), dtype=torch.uint8, device=dev)
        fe.interpolate_multi_device_stream(d_frames.data_ptr(), c.n, w, h, list(TIMES), mid.data_ptr(), fl.data_ptr() if c.flows else 0, 0,
                                           _stream(), flow_format=c.ffmt)
    out = {"mid": fetch(mid), "flows": fetch(fl)}
    if not c.flows:  # no flow buffer was given: nothing was stored there
        assert np.isnan(out["flows"].astype(np.float32)).all(), case_id(c)
    return out


def _assert_same_bytes(got, want, tag):
    assert sorted(got) == sorted(want), tag
    for name in want:
        g, x = got[name], want[name]
        assert g.dtype == x.dtype and g.shape == x.shape, (tag, name, g.dtype, g.shape, x.shape)
        diff = g.view(np.uint8) != x.view(np.uint8)
        if diff.any():
            cells = np.argwhere(diff.reshape(g.shape + (-1,)).any(axis=-1))
            with np.errstate(invalid="ignore"):
                worst = float(np.nanmax(np.abs(g.astype(np.float64) - x.astype(np.float64))))
            first = tuple(int(v) for v in cells[0])
            raise AssertionError(f"{tag}: '{name}' differs in {len(cells)} of {g.size} elements, max |difference| {worst:.3g}"
                                 f"{'' if np.isfinite(g.astype(np.float64)).all() else ' (not every element is finite)'}, first at (.., y, x, c) "
                                 f"{first}: got {g[first]!r}, want {x[first]!r}")


def times_of(c):
    return [T_ONE] if c.entry == IDS else list(TIMES)


_SELECT_FRAMES = {}  # (what select_frames depends on) -> frames, read-only


def select_frames(nsc, c):
    """What an EXACT handle with the setting on owes for its in-between frames, (n - 1, times, h, w, 4): the CPU restatement of
    each pair's forward and backward flow, rounded to f16 where the hand-off is Rg16Float, uploaded and run through
    nus_interp_interpolate_select_device in FMA mode with the handle's projection rounds (the header's statement of the setting;
    tests/test_gpu_flow_select_forms.py holds that entry point to its own restatement).  The backward flow never leaves the
    workspace: this is what makes it answerable to the CPU.  (A cut pair's frames are the select warp's here: _assert_cut_pair.)"""
    import torch

    key = (c.size, c.n, c.scene, c.steps, c.warps, c.median, c.project, c.ffmt, tuple(times_of(c)))
    if key not in _SELECT_FRAMES:
        w, h = c.size
        times = times_of(c)
        fields = [np.stack([_restated(c.size, c.n, c.scene, c.steps, c.warps, c.median, k, back) for k in range(c.n - 1)]) for back in (False, True)]
        if c.ffmt == "f16":
            fields = [f.astype(np.float16) for f in fields]
        d_frames, d_fwd, d_bwd = put(_frames(c.size, c.n, c.scene), "cuda:0"), put(fields[0]), put(fields[1])
        warp = nsc.WgpuFrameInterpolator()
        warp.set_mode("fma"), warp.set_flow_format(c.ffmt), warp.set_flow_project(c.project)
        fb = w * h * 4
        out = guarded.empty((c.n - 1, len(times), h, w, 4), dtype=torch.uint8, device="cuda:0")
        warp.interpolate_select_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_fwd.data_ptr(), d_bwd.data_ptr(), w, h, times,
                                       out.data_ptr(), 0, c.n - 1, _stream())
        _SELECT_FRAMES[key] = _frozen(fetch(out))
    return _SELECT_FRAMES[key]


def assert_select_frames(nsc, c, out):
    """The frames of a call with the setting on against select_frames, byte for byte (a cut pair's are repeats: _assert_cut_pair)."""
    want = select_frames(nsc, c)
    got = out["mid"].reshape(want.shape)
    pairs = [k for k in range(c.n - 1) if not (c.scene and k == 2)]
    if not np.array_equal(got[pairs], want[pairs]):
        diff = got[pairs] != want[pairs]
        first = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{case_id(c)}: the frames are not the select warp's of the restated forward and backward flows: {int(diff.sum())} "
                             f"of {diff.size} bytes differ in pairs {sorted({pairs[i] for i in np.argwhere(diff)[:, 0]})}, largest difference "
                             f"{int(np.abs(got[pairs].astype(int) - want[pairs]).max())}, first at (pair, time, y, x, c) {first}")


def _assert_restated(c, out, nsc=None):
    """EXACT: the flows are the float32 restatement's (values where a median ran: a selection may return either zero), the
    Rg16Float flows its rounding to nearest even; a primitive's result is its restatement's.  With the setting on also the frames:
    assert_select_frames."""
    tag = case_id(c)
    if c.bidir:
        assert_select_frames(nsc, c, out)
    if c.entry in PRIMITIVES:
        want = _primitive_reference(c.entry, c.size, c.steps[1])
        got = out["out"]
        assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.shape, want.shape)
        if c.entry in ("median3", "median5", "project_flow"):
            assert np.array_equal(got, want), (tag, float(np.abs(got - want).max()))
        else:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, float(np.abs(got - want).max()))
        return
    if c.entry in ESTIMATORS[3:] and not c.flows:
        return  # (the flows stayed in the workspace; the frames are held to the first call's and the fresh handle's)
    n_pairs = 1 if c.entry in ("estimate", "estimate_device") else c.n - 1
    want = np.stack([_restated(c.size, c.n, c.scene, c.steps, c.warps, c.median, k) for k in range(n_pairs)])
    got = out["flows"]
    if c.ffmt == "f16":
        want = want.astype(np.float16)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    if c.median:
        same = np.array_equal(got, want)
    else:
        same = np.array_equal(got.view(np.uint8), want.view(np.uint8))
    if not same:
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64))))
        raise AssertionError(f"{tag}: the flows are not the float32 restatement's, max |difference| {worst:.3g} px, "
                             f"{int((got != want).sum())} of {got.size} values")


def _assert_cut_pair(c, out):
    """Scene detection on: the cut pair's in-between frames are repeats of the nearer real frame, the other pairs' are not."""
    w, h = c.size
    frames = _frames(c.size, c.n, True)
    cut = [bool(sc.is_cut(*sc.measures(frames[k], frames[k + 1]), w, h)) for k in range(c.n - 1)]
    assert cut == [k == 2 for k in range(c.n - 1)], cut
    for j, t in enumerate(TIMES):
        assert np.array_equal(out["mid"][2, j], frames[2] if t < 0.5 else frames[3]), (case_id(c), j)
        assert not np.array_equal(out["mid"][1, j], frames[1]) and not np.array_equal(out["mid"][1, j], frames[2]), (case_id(c), j)
    assert c.entry == IMS  # (scene detection is the multi-time entry point's)


# ---- the lattice ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_poisoned_workspace(nsc, monkeypatch, c):
    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    if c.chunk:
        monkeypatch.setenv(CHUNK_ENV, str(c.chunk))
    else:
        monkeypatch.delenv(CHUNK_ENV, raising=False)
    tag = case_id(c)
    d = None if c.entry in PRIMITIVES else put(_frames(c.size, c.n, c.scene), "cuda:0")
    fresh = _call(_estimator(nsc, c), c, d)
    fe = _estimator(nsc, c)
    first = _call(fe, c, d)  # primes the handle: the workspace reaches its size
    reserved = fe.workspace_bytes
    assert reserved > 0, tag
    caught = {}  # every comparison is made before the verdict: which fill bytes catch a defect is what there are four for

    def hold(key, got, want, what):
        try:
            _assert_same_bytes(got, want, (tag, what))
        except AssertionError as e:
            caught[key] = str(e)

    hold("fresh handle", first, fresh, "the first call against a fresh handle's")
    for byte in BYTES:
        fe._fill_workspace(byte, _stream())
        again = _call(fe, c, d)
        assert fe.workspace_bytes == reserved, (tag, hex(byte), fe.workspace_bytes, reserved)  # no unpoisoned growth inside a repeat
        hold(f"{byte:#04x}", again, first, f"after a fill with {byte:#04x} against the first call's")
    assert not caught, f"{tag}: the result depends on what the workspace held -- caught by {sorted(caught)}:\n" + "\n".join(caught.values())
    for name, a in first.items():  # nothing the call left is a NaN but the buffer it was not given
        if name != "flows" or c.flows:
            assert np.isfinite(a.astype(np.float64)).all(), (tag, name)
    if c.mode == "exact":
        _assert_restated(c, first, nsc)
    if c.scene:
        _assert_cut_pair(c, first)
    if d is not None:
        assert np.array_equal(fetch(d), _frames(c.size, c.n, c.scene)), tag  # the frames are inputs
    # for the census
    if c.entry in PRIMITIVES:
        _SEEN.add(c.entry)
        if c.entry.startswith("horn_schunck"):
            _SEEN.add((c.entry.split("+")[0], c.tiled))
        return
    path = path_of(c)  # (with the setting on: a path of its own)
    _SEEN.update({("warps", c.warps, path), ("median", c.median, path), ("project", c.project, path)})
    if c.bidir:  # entries of their own: a case with the setting on stands in for no case with it off
        _SEEN.update({("bidir", c.entry, c.tiled, c.mode), ("bidir", c.ffmt, c.flows)})
        if c.chunk:
            assert c.n - 1 == 5 and c.chunk == 2  # chunks of 2, 2 and 1 pairs
            _SEEN.add(("bidir", "chunked", c.entry))
        if c.scene:
            _SEEN.add(("bidir", "scene", c.entry))
        return
    _SEEN.add((c.entry, c.tiled, c.mode))
    if c.entry in ESTIMATORS[3:]:
        _SEEN.add((c.entry, c.ffmt, c.flows))
    if c.chunk:
        assert c.n - 1 == 5 and c.chunk == 2  # chunks of 2, 2 and 1 pairs
        _SEEN.add(("chunked", c.ffmt, c.flows, c.entry))
    if c.scene:
        _SEEN.add(("scene", c.entry))
    levels, coarse, refine = c.steps
    for name, hit in (("coarse_iters 0", coarse == 0), ("refine_iters 0", refine == 0), ("levels 1", levels == 1),
                      ("two launches a level", coarse > 8 or refine > 5), ("4 levels", levels == 4)):
        if hit:
            _SEEN.add((name, path))
    _SEEN.add(("size", c.size))


# ---- history without poison, across the slot aliases ------------------------------------------------------------------------------
# (A, B) per row: on one handle A, B, A.  B crosses a boundary the slots share with A.
HISTORY = {
    # kLum of the batch path, then the same memory as the primitive's coefficient planes (kPyrA)
    "batch-then-horn_schunck": (C("estimate_device_stream", S97, (3, 9, 6), 1, n=5), C("horn_schunck", S97, tiled=1)),
    # kCoef then frame B's pyramid (kPyrB); kLevelInEven then the pair path's coefficients (kTemp)
    "warped-batch-then-pair": (C("estimate_device_stream", S97, (3, 9, 6), 1, warps=2, n=5), C("estimate_device", S97, (3, 9, 6), 1, warps=2)),
    # the level offsets inside the pyramid slots move
    "pair-160x96-then-stream-97x61-L4": (C("estimate_device", S160, (3, 9, 6), 1, warps=2), C("estimate_device_stream", S97, (4, 11, 3), 1, n=5)),
    # the fast pyramid's one float per pixel, then f32 RGBA levels in the same slots
    "fast-streamed-then-exact-per-step": (C("estimate_device_stream", S97, (3, 9, 6), 3, "fast", n=5), C("estimate_device_stream", S97, (3, 9, 6), 0, n=5)),
    # the halves beside the flows, then f32 flows in the caller's buffer
    "f16-noflows-then-f32-flows": (C(IDS, S160, tiled=1, n=4, ffmt="f16", flows=False), C(IDS, S160, tiled=1, n=4, ffmt="f32", flows=True)),
    # the setting on, off, on: its three slots are released and reserved again
    "bidir-on-off-on": (C(IMS, S160, tiled=1, warps=2, project=2, n=4, ffmt="f32", flows=False, bidir=True),
                        C(IMS, S160, tiled=1, warps=2, project=2, n=4, ffmt="f32", flows=False)),
    # kFwdFlows and kBwdFlows hold halves, then kBwdFlows f32 flows and the forward flows go to the caller
    "bidir-f16-noflows-then-f32-flows": (C(IDS, S160, tiled=1, n=4, ffmt="f16", flows=False, bidir=True),
                                         C(IDS, S160, tiled=1, n=4, ffmt="f32", flows=True, bidir=True)),
    # kBwdFlows: the chunk's halves, then one pair's f32 flow with its halves behind it
    "bidir-batch-then-pair-by-pair": (C(IMS, S160, tiled=1, median=3, n=4, ffmt="f16", flows=True, bidir=True),
                                      C(IMS, S160, tiled=0, median=3, n=4, ffmt="f16", flows=True, bidir=True)),
}


def _set(fe, c):
    """The settings of case c on a used handle."""
    fe.levels, fe.coarse_iterations, fe.refine_iterations = c.steps
    fe.set_warps(c.warps), fe.set_median(c.median), fe.set_project(c.project), fe.set_mode(c.mode), fe.set_tiled(c.tiled)
    fe.set_bidirectional(c.bidir)


@pytest.mark.parametrize("name", sorted(HISTORY), ids=str)
def test_history_across_the_slot_aliases(nsc, monkeypatch, name):
    import torch

    monkeypatch.delenv(CHUNK_ENV, raising=False)
    a, b = HISTORY[name]
    dev = {c: None if c.entry in PRIMITIVES else put(_frames(c.size, c.n, c.scene), "cuda:0") for c in (a, b)}
    fresh = {c: _call(_estimator(nsc, c), c, dev[c]) for c in (a, b)}
    fe = _estimator(nsc, a)
    held = 0
    for stop, c in enumerate((a, b, a)):
        _set(fe, c)
        torch.cuda.synchronize()  # the stream rule: a host entry point (and nothing else here) needs it
        got = _call(fe, c, dev[c])
        _assert_same_bytes(got, fresh[c], (name, f"stop {stop}", case_id(c)))
        if stop and (a, b, a)[stop - 1].bidir and not c.bidir:  # turning the setting off is the one thing that gives memory back
            assert 0 < fe.workspace_bytes < held, (name, stop, fe.workspace_bytes, held)
        else:
            assert fe.workspace_bytes >= held > 0 or stop == 0, (name, stop, fe.workspace_bytes, held)  # grow-only
        held = fe.workspace_bytes
    for c in (a, b):
        if c.mode == "exact":
            _assert_restated(c, fresh[c], nsc)


# ---- the stream rule ----------------------------------------------------------------------------------------------------------------
def _two_calls():
    """Two streams of flows of different shape, content and settings' reach: 4 pairs of 97 x 61, 3 pairs of 64 x 48."""
    return C("estimate_device_stream", S97, (3, 9, 6), 1, warps=2, n=5), C("estimate_device_stream", S64, (3, 9, 6), 1, warps=2, n=4)


@pytest.mark.parametrize("how", ["primed", "primed-and-poisoned", "second-call-grows"])
def test_calls_on_one_stream_need_no_synchronisation(nsc, monkeypatch, how):
    """nuscaler_hip.h, "THE STREAM RULE": calls of one handle enqueued on ONE stream need nothing between them.  Both calls and
    the fills of their output buffers go to one non-default stream, the host waits once, behind the second call.  "grows": the
    handle has only seen the small call, so the large one frees and reallocates slots the small one may still be running in --
    reserve() waits for the caller's stream before it frees."""
    import torch

    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    monkeypatch.delenv(CHUNK_ENV, raising=False)
    big, small = _two_calls()
    order = (small, big) if how == "second-call-grows" else (big, small)
    fresh = {}
    for c in order:
        fresh[c] = _call(_estimator(nsc, c), c, put(_frames(c.size, c.n), "cuda:0"))["flows"]
    fe = _estimator(nsc, big)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        assert s != 0 and s == _stream()
        dev = {c: put(_frames(c.size, c.n), "cuda:0") for c in order}
        for c in (order[:1] if how == "second-call-grows" else order):  # prime
            _call(fe, c, dev[c])
        primed = fe.workspace_bytes
        if how == "primed-and-poisoned":
            fe._fill_workspace(0xFF, s)
        outs = []
        for c in order:  # back to back: no fetch, no synchronisation in between
            out = guarded.full((c.n - 1, c.size[1], c.size[0], 2), float("nan"), dtype=torch.float32, device="cuda:0")
            fe.estimate_device_stream(dev[c].data_ptr(), c.n, c.size[0], c.size[1], out.data_ptr(), s)
            outs.append(out)
        stream.synchronize()  # the one wait
        got = [fetch(o) for o in outs]
    if how == "second-call-grows":
        assert fe.workspace_bytes > primed > 0
    else:
        assert fe.workspace_bytes == primed > 0  # the second call did not grow the workspace
    for c, g in zip(order, got):
        _assert_same_bytes({"flows": g}, {"flows": fresh[c]}, (how, case_id(c)))
    _assert_restated(big, {"flows": fresh[big]})
    _assert_restated(small, {"flows": fresh[small]})


def test_bidirectional_calls_on_one_stream_need_no_synchronisation(nsc, monkeypatch):
    """The stream rule with the setting on: two calls of different shape on one non-default stream with nothing between them, the
    second growing the workspace -- kFwdFlows, kBwdFlows and kBwdCoef among the slots it frees while the first may still run in them."""
    import torch

    monkeypatch.delenv(CHUNK_ENV, raising=False)
    small = C(IMS, S64, tiled=1, warps=2, project=2, n=4, ffmt="f16", flows=False, bidir=True)
    big = C(IMS, S97, tiled=1, warps=2, project=2, n=5, ffmt="f16", flows=False, bidir=True)
    fresh = {c: _call(_estimator(nsc, c), c, put(_frames(c.size, c.n), "cuda:0"))["mid"] for c in (small, big)}
    fe = _estimator(nsc, small)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        assert s != 0 and s == _stream()
        dev = {c: put(_frames(c.size, c.n), "cuda:0") for c in (small, big)}
        _call(fe, small, dev[small])  # prime: the handle has seen the small call only
        primed = fe.workspace_bytes
        outs = []
        for c in (small, big):  # back to back: no fetch, no synchronisation in between
            out = guarded.empty((c.n - 1, len(TIMES), c.size[1], c.size[0], 4), dtype=torch.uint8, device="cuda:0")
            fe.interpolate_multi_device_stream(dev[c].data_ptr(), c.n, c.size[0], c.size[1], list(TIMES), out.data_ptr(), 0, 0, s, flow_format=c.ffmt)
            outs.append(out)
        stream.synchronize()  # the one wait
        got = [fetch(o) for o in outs]
    assert fe.workspace_bytes > primed > 0
    for c, g in zip((small, big), got):
        _assert_same_bytes({"mid": g}, {"mid": fresh[c]}, ("bidirectional, second call grows", case_id(c)))
        assert_select_frames(nsc, c, {"mid": fresh[c]})


# ---- the census ---------------------------------------------------------------------------------------------------------------------
def test_every_entry_was_held_with_a_poisoned_workspace():
    """Runs last: what the lattice above saw is what the handle can be asked for."""
    want = set(PRIMITIVES)
    want |= {(e, tiled, "exact") for e in ESTIMATORS for tiled in (0, 1, 2, 3)} | {(e, tiled, "fast") for e in ESTIMATORS for tiled in (1, 3)}
    want |= {(e, ffmt, flows) for e in (IDS, IMS) for ffmt in ("f32", "f16") for flows in (True, False)}
    want |= {("chunked", ffmt, flows, IDS) for ffmt in ("f32", "f16") for flows in (True, False)}
    want |= {(setting, v, path) for setting, values in (("warps", (0, 2)), ("median", (0, 3, 5)), ("project", (0, 2))) for v in values
             for path in (PAIR, BATCH, PER_STEP)}
    want |= {(name, path) for name in ("coarse_iters 0", "refine_iters 0", "two launches a level") for path in (PAIR, BATCH, PER_STEP)}
    want |= {("levels 1", PAIR), ("levels 1", BATCH), ("4 levels", PAIR), ("4 levels", BATCH)}
    want |= {("scene", IMS)}
    # the setting on: every reachable entry x set_tiled x mode, both hand-offs with and without a flow buffer, chunks, a cut, and
    # every setting on both roads of the backward solve
    want |= {("bidir", e, tiled, "exact") for e in (IDS, IMS) for tiled in (0, 1, 2, 3)} | {("bidir", e, tiled, "fast") for e in (IDS, IMS) for tiled in (1, 3)}
    want |= {("bidir", ffmt, flows) for ffmt in ("f32", "f16") for flows in (True, False)}
    want |= {("bidir", "chunked", IDS), ("bidir", "scene", IMS)}
    want |= {(setting, v, path + BACKWARD) for setting, values in (("warps", (0, 2)), ("median", (0, 3, 5)), ("project", (0, 2))) for v in values
             for path in (BATCH, PER_STEP)}
    want |= {("horn_schunck", t) for t in (0, 1, 2, 3)} | {("horn_schunck_coef", t) for t in (1, 2, 3)}
    want |= {("size", s) for s in (S97, S64, S33, S160)}
    missing = sorted(map(str, want - _SEEN))
    assert not missing, missing
    print(f"{len(CASES)} cases x {len(BYTES)} fill bytes; {len(_SEEN)} census entries")
