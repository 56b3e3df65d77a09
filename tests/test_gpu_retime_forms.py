"""The rate conversion's kernel forms, strides and launch split on the MI355X: what test_gpu_retime.py and
test_gpu_retime_streams.py, which hold the dense-flow route at small sizes, never launch.

  block vectors   nus_bm_retime_device_stream at the smallest frames that select each of k_retime_warp_tiny<kTinyBlocks> and the four
                  k_retime_bm<MODE, XV> table entries, in both modes: the vectors are nus_bm_estimate_device's, every in-between
                  output is nus_bm_warp_device's at t_j and -- sharing no device code with the conversion -- the oracle's warp of the
                  expanded vectors (EXACT: equal; FMA: tests/_warp64.py's contract), gapped input and output strides.
  cut rule        nus_scene_apply_cuts_retime_device against numpy, in the 16-byte form and, by size, stride and base, the scalar one.
  launch split    66 000 pairs of a few pixels through every launcher that advances more than the frames at the 65 535-pair split:
                  whole call against two calls that do not cross it, and the probe pairs against the oracle on the host.

Every case asserts the host-side condition that selects its kernel, so a later change of a size cannot move it to another kernel
unnoticed.  Every device output comes from conftest.guarded with a poison fill."""
import functools

import numpy as np
import pytest

import _blockmatch as bmref
import _flow_project as PJ
import _retime
from _warp64 import warp_contract
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

POISON = 0x6D
N = 5
BM_RATIOS = [(5, 2), (2, 5), (12, 5), (1, 1), (8, 1)]
# (w, h, block size, bidirectional, the kernel form): the smallest frames that select each form; 34 x 18 has several blocks per row
# and a ragged last block at block size 8 and 16
BM_CASES = [(1, 1, 8, False, "tiny"), (1, 5, 8, False, "tiny"), (7, 1, 8, False, "tiny"), (7, 5, 8, False, "xv1"), (33, 17, 8, False, "xv1"),
            (8, 6, 8, False, "xv2"), (34, 18, 8, False, "xv2"), (34, 18, 16, False, "xv2"), (33, 17, 8, True, "xv1"), (34, 18, 8, True, "xv2")]

_oracle = None


@pytest.fixture(autouse=True)
def _bind_oracle(oracle_mod):
    global _oracle
    _oracle = oracle_mod


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _aligned16(t):
    return (t.data_ptr() + 15) & ~15


def _eps(w, h):
    return 0.5 if min(w, h) >= 2 else 1.0  # (frames below 2 x 2 run EXACT arithmetic: tests/test_gpu_bm_warp.py)


# ---- A. block vectors --------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _bm_frames(w, h):
    """(N, h, w, 4), read-only: noise, each frame the one before moved by a few pixels with its low bits disturbed -- the search
    finds vectors that are not zero and differ from pair to pair."""
    rng = np.random.default_rng(4100 + 31 * w + h)
    f = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8)]
    for dx, dy in [(3, -2), (-1, 1), (2, 3), (-4, 0)]:
        f.append(np.roll(f[-1], (dy, dx), (0, 1)) ^ rng.integers(0, 4, (h, w, 4), dtype=np.uint8))
    f = np.stack(f)
    f.setflags(write=False)
    return f


def _strided(frames, gap, fill):
    n = len(frames)
    fb = frames[0].size
    buf = np.full((n, fb + gap), fill, np.uint8)
    buf[:, :fb] = frames.reshape(n, fb)
    return buf


def _bm_estimate(bm, d_frames, stride, w, h):
    """The vectors nus_bm_estimate_device writes for the stream's N - 1 pairs, int16 (N - 1, blocks_y, blocks_x, 2)."""
    import torch

    need = bm.workspace_size(w, h, N - 1)
    ws = guarded.empty((need + 16,), dtype=torch.uint8, device="cuda:0")
    nbx, nby = bm.block_grid(w, h)
    vec = guarded.full((N - 1, nby, nbx, 2), 0x7B7B, dtype=torch.int16, device="cuda:0")
    bm.estimate_device(d_frames, stride, d_frames + stride, stride, w, h, N - 1, _aligned16(ws), need, vec.data_ptr(), stream=_stream())
    return fetch(vec)


def _bm_convert(bm, d_frames, stride, w, h, num, den, mode, out_gap, form):
    """-> (frames (n_out, h, w, 4), the output gaps' bytes, the device tensor of the vectors).  Asserts the kernel form."""
    import torch

    fb = w * h * 4
    n_out = _retime.count(N, num, den)
    ws_bytes = bm.stream_workspace_size(w, h, N)
    ws = guarded.empty((ws_bytes + 16,), dtype=torch.uint8, device="cuda:0")
    nbx, nby = bm.block_grid(w, h)
    vec = guarded.full((N - 1, nby, nbx, 2), 0x7B7B, dtype=torch.int16, device="cuda:0")
    out = guarded.full((n_out, fb + out_gap), POISON, dtype=torch.uint8, device="cuda:0")
    # launch_retime_warp: the tiny kernel below 2 px either way; else kernels[fma][pair_ok]
    tiny = w < 2 or h < 2
    pair_ok = w % 2 == 0 and out.data_ptr() % 8 == 0 and (fb + out_gap) % 8 == 0
    assert ("tiny" if tiny else "xv2" if pair_ok else "xv1") == form, (w, h, out_gap, form)
    bm.retime_stream_device(d_frames, stride, N, w, h, num, den, _aligned16(ws), ws_bytes, out.data_ptr(), mode=mode,
                            d_vectors=vec.data_ptr(), out_frame_stride=fb + out_gap if out_gap else 0, stream=_stream())
    raw = fetch(out)
    return raw[:, :fb].reshape(n_out, h, w, 4), raw[:, fb:], vec


def _bm_check(bm, frames, d_frames, stride, w, h, bs, num, den, mode, want_vec, out_gap=0, form=None):
    """One conversion held to checks 1 - 3 of the module docstring.  -> (frames, vectors)"""
    import torch

    fb = w * h * 4
    tag = (w, h, bs, num, den, mode, out_gap)
    got, gaps, d_vec = _bm_convert(bm, d_frames, stride, w, h, num, den, mode, out_gap, form)
    assert (gaps == POISON).all(), (tag, "an output gap was written")
    vec = fetch(d_vec)
    assert np.array_equal(vec, want_vec), (tag, "d_vectors is not nus_bm_estimate_device's")
    sched = _retime.schedule(N, num, den)
    assert len(got) == len(sched)
    nb = vec.shape[1] * vec.shape[2]
    sib = guarded.full((len(sched), h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
    for j, (k, r, t) in enumerate(sched):
        if r != 0:
            a = d_frames + k * stride
            bm.warp_device(a, stride, a + stride, stride, w, h, 1, d_vec.data_ptr() + k * nb * 4, sib.data_ptr() + j * fb, times=[float(t)],
                           mode=mode, stream=_stream())
    sib = fetch(sib)
    for j, (k, r, t) in enumerate(sched):
        if r == 0:
            assert np.array_equal(got[j], frames[k]), (tag, j, "a real-frame output is not the input frame")
            continue
        assert np.array_equal(got[j], sib[j]), (tag, j, k, float(t), "differs from nus_bm_warp_device at t_j")
        a, b = frames[k], frames[k + 1]
        flow = bmref.dense_flow(vec[k], w, h, bs)
        if mode == "exact":
            host = np.frombuffer(bm.interpolate(a, b, w, h, times=[float(t)], mode="exact")[0], np.uint8)
            assert np.array_equal(got[j].reshape(-1), host), (tag, j, k, float(t), "differs from nus_bm_interpolate")
            assert np.array_equal(got[j], _oracle.warp_blend(a, b, flow, float(t))), (tag, j, k, float(t), "differs from the oracle")
        else:
            warp_contract(got[j], a, b, flow, np.float32(t), _eps(w, h), ("bm retime", tag, j))
    return got, vec


@pytest.mark.parametrize("mode", ["exact", "fma"])
@pytest.mark.parametrize("w,h,bs,bidir,form", BM_CASES)
def test_block_vector_conversion_in_every_kernel_form(nsc, w, h, bs, bidir, form, mode):
    """The only test to launch k_retime_warp_tiny<kTinyBlocks> ("tiny"), k_retime_bm<Exact, 2>, k_retime_bm<Fma, 1> and
    k_retime_bm<Fma, 2> ("xv1" / "xv2" by width parity), the only one of nus_bm_retime_device_stream in FMA mode and the only one to
    read its d_vectors back; k_retime_bm<Exact, 1> is here too.  The oracle's warp of the expanded vectors is the one check of the
    conversion that shares no device code with it."""
    frames = _bm_frames(w, h)
    fb = w * h * 4
    d = put(np.ascontiguousarray(frames))
    bm = nsc.BlockMatcher(block_size=bs, search_radius=6, bidirectional=bidir)
    want_vec = _bm_estimate(bm, d.data_ptr(), fb, w, h)
    if min(w, h) >= 17:  # (a single partial block has no candidate but 0; the forward-backward check may zero a pair's field)
        moving = [bool(v.any()) for v in want_vec]
        assert any(moving) if bidir else all(moving), (moving, "these frames move: a stream of zero fields would test no sampling")
    for num, den in BM_RATIOS:
        _bm_check(bm, frames, d.data_ptr(), fb, w, h, bs, num, den, mode, want_vec, form=form)


@pytest.mark.parametrize("mode", ["exact", "fma"])
def test_block_vector_conversion_with_gapped_input_and_output(nsc, mode):
    """nus_bm_retime_device_stream with frame_stride and out_frame_stride above a frame (b = a + frame_stride and the search's
    strides; RetimeTimes' stride): the bytes and the vectors are the tight call's, poison in the input gaps is never read -- another
    poison changes no byte -- and the output gaps keep theirs.  A gap of 16 keeps k_retime_bm<MODE, 2>; a gap of 4 on the same
    even-width frame turns pair_ok off through out_frame_stride % 8: k_retime_bm<MODE, 1> where the pair form would fit."""
    w, h, bs = 34, 18, 8
    frames = _bm_frames(w, h)
    fb = w * h * 4
    bm = nsc.BlockMatcher(block_size=bs, search_radius=6)
    tight = put(np.ascontiguousarray(frames))
    want_vec = _bm_estimate(bm, tight.data_ptr(), fb, w, h)
    in_gap = 20
    gapped = [put(_strided(frames, in_gap, fill)) for fill in (0xE1, 0x1E)]
    assert np.array_equal(_bm_estimate(bm, gapped[0].data_ptr(), fb + in_gap, w, h), want_vec)
    for num, den in [(5, 2), (12, 5)]:
        want, _ = _bm_check(bm, frames, tight.data_ptr(), fb, w, h, bs, num, den, mode, want_vec, form="xv2")
        for out_gap, form in ((16, "xv2"), (4, "xv1")):
            got0, _ = _bm_check(bm, frames, gapped[0].data_ptr(), fb + in_gap, w, h, bs, num, den, mode, want_vec, out_gap, form)
            got1, _, d_vec = _bm_convert(bm, gapped[1].data_ptr(), fb + in_gap, w, h, num, den, mode, out_gap, form)
            assert np.array_equal(got0, want), (mode, num, den, out_gap, "the gapped call differs from the tight one")
            assert np.array_equal(got1, got0) and np.array_equal(fetch(d_vec), want_vec), (mode, num, den, out_gap, "an input gap was read")
    for g, fill in zip(gapped, (0xE1, 0x1E)):
        assert np.array_equal(fetch(g), _strided(frames, in_gap, fill)), "the input stream was written"


# ---- B. the cut rule ---------------------------------------------------------------------------------------------------------------


def _as_rgba(frames, fmt):
    """The copy nus_scene_apply_cuts_device defines for `fmt` (0 RGBA, 1 BGRA, 2 RGBX, 3 BGRX): channel order to RGBA, alpha 255 for X."""
    out = np.array(frames[..., [2, 1, 0, 3]] if fmt in (1, 3) else frames)
    if fmt in (2, 3):
        out[..., 3] = 255
    return out


def _cut_reference(frames, cut, num, den, fmt, first=0, count=None):
    """Outputs first .. first + count - 1 of the stream after the cut rule alone, in numpy: the copy of frame k_j (t_j < 0.5) or
    k_j + 1 where pair k_j is cut and r_j != 0; POISON everywhere else."""
    tbl = _retime.schedule_array(len(frames), num, den, first, count)
    k, r, t = tbl[:, 0].astype(np.int64), tbl[:, 1], _retime.times_of(tbl)
    hit = r != 0
    hit[hit] = cut[k[hit]] != 0
    src = np.where(t < np.float32(0.5), k, k + 1)
    want = np.full((len(tbl),) + frames.shape[1:], POISON, np.uint8)
    want[hit] = _as_rgba(frames, fmt)[src[hit]]
    return want


def _apply_cuts(nsc, d_frames, stride, n, w, h, fmt, num, den, d_cut, d_out, out_stride=0):
    st = nsc._capi.lib().nus_scene_apply_cuts_retime_device(d_frames, stride, n, w, h, fmt, num, den, d_cut, d_out, out_stride, _stream())
    assert st == 0, nsc._capi.last_error()


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", [(8, 6), (7, 5)])
def test_cut_rule_on_the_schedule_in_both_streaming_forms(nsc, w, h, fmt):
    """nus_scene_apply_cuts_retime_device against numpy.  8 x 6 (48 px, bases and strides on 16 bytes) is the only direct test of
    k_retime_scene_apply<true>; 7 x 5 takes k_retime_scene_apply<false> by size, and 8 x 6 with frame_stride = fb + 4, or with d_out
    4 bytes up, takes it by stride or base (stream_shape) and must write the same frames.  Cut and uncut neighbours, a cut on the
    first and on the last pair; outputs of uncut pairs and real frames keep their poison."""
    import torch

    n = 7
    cut = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    rng = np.random.default_rng(88 + w)
    frames = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    fb = w * h * 4
    d_tight, d_gapped, d_cut = put(frames), put(_strided(frames, 4, 0xE1)), put(cut)
    for num, den in [(12, 5), (2, 5), (3, 1)]:
        n_out = _retime.count(n, num, den)
        want = _cut_reference(frames, cut, num, den, fmt)
        assert (want != POISON).any() or (num, den) == (2, 5)
        results = {}
        for form, (d_in, stride, off) in {"tight": (d_tight, fb, 0), "in4": (d_gapped, fb + 4, 0), "out4": (d_tight, fb, 4)}.items():
            buf = guarded.full((n_out * fb + 2 * off,), POISON, dtype=torch.uint8, device="cuda:0")
            vec = (w * h) % 4 == 0 and stride % 16 == 0 and d_in.data_ptr() % 16 == 0 and (buf.data_ptr() + off) % 16 == 0  # stream_shape
            assert vec == ((w, h) == (8, 6) and form == "tight"), (w, h, form)
            _apply_cuts(nsc, d_in.data_ptr(), stride, n, w, h, fmt, num, den, d_cut.data_ptr(), buf.data_ptr() + off)
            raw = fetch(buf)
            assert (raw[:off] == POISON).all() and (raw[len(raw) - off:] == POISON).all(), (form, "a byte outside the stream was written")
            results[form] = raw[off:len(raw) - off].reshape(n_out, h, w, 4)
            bad = [j for j in range(n_out) if not np.array_equal(results[form][j], want[j])]
            assert not bad, (w, h, fmt, num, den, form, bad)


# ---- D. the launch split at 65 535 pairs ---------------------------------------------------------------------------------------------

N_PAIRS, SPLIT = 66000, 65535
PROBES = [0, 1, SPLIT - 1, SPLIT, SPLIT + 1, N_PAIRS - 1]
SPLIT_SIZES = [(4, 2), (3, 2), (2, 1)]  # the tile's pixel-pair form, its one-pixel form, the tiny kernels
T = float(np.float32(0.37))


@functools.lru_cache(maxsize=None)
def _split_content(w, h):
    """(frames (N_PAIRS + 1, h, w, 4), flows (N_PAIRS, h, w, 2) f32, cut flags (N_PAIRS,)), read-only and random throughout: an
    offset that forgets the pairs already launched cannot land on equal data."""
    rng = np.random.default_rng(6500 + 31 * w + h)
    frames = rng.integers(0, 256, (N_PAIRS + 1, h, w, 4), dtype=np.uint8)
    flows = rng.uniform(-2.5, 2.5, (N_PAIRS, h, w, 2)).astype(np.float32)
    cut = rng.integers(0, 2, N_PAIRS, dtype=np.uint8)
    for a in (frames, flows, cut):
        a.setflags(write=False)
    return frames, flows, cut


def _interp(nsc, mode, ffmt, rounds):
    it = nsc.WgpuFrameInterpolator()
    it.set_mode(mode), it.set_flow_format(ffmt), it.set_flow_project(rounds)
    return it


def _as_read(flows, ffmt):
    """(what goes to the device, the f32 values the warp reads)"""
    if ffmt == "f16":
        half = flows.astype(np.float16)
        return half, half.astype(np.float32)
    return flows, flows


def _oracle_frame(frames, seen, k, t, rounds):
    """The oracle's in-between frame of pair k at t: warp_blend of the flow as the warp reads it, projected first (0 rounds: as it is);
    seen None: zero flow."""
    flow = None if seen is None else PJ.project_f32(seen[k], t, rounds) if rounds else seen[k]
    return _oracle.warp_blend(frames[k], frames[k + 1], flow, float(t))


def _assert_pair_form(w, h, *pointers_and_strides):
    """The (w, h) of SPLIT_SIZES select the forms their comment names: 4 x 2 with everything given on 16 bytes is the pair form."""
    assert (w >= 2 and h >= 2) == ((w, h) != (2, 1))
    assert (w % 2 == 0 and h >= 2) == ((w, h) == (4, 2))
    if (w, h) == (4, 2):
        assert all(v % 16 == 0 for v in pointers_and_strides), pointers_and_strides


@pytest.mark.parametrize("rounds", [0, 1])
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", SPLIT_SIZES)
def test_single_time_warp_across_the_launch_split(nsc, w, h, ffmt, rounds):
    """nus_interp_interpolate_device over 66 000 pairs WITH a flow: the only test in which the chunk lambdas of launch_warp_blend
    (rounds 0) and launch_warp_blend_project (rounds 1) advance the flow plane by `done` -- test_more_frames_than_one_grid_axis_holds
    crosses the split with zero flow only."""
    import torch

    frames, flows, _ = _split_content(w, h)
    dev, seen = _as_read(flows, ffmt)
    fb, plane = w * h * 4, w * h * dev.itemsize * 2
    d_frames, d_flows = put(frames), put(np.ascontiguousarray(dev))
    _assert_pair_form(w, h, d_frames.data_ptr(), d_flows.data_ptr(), fb, plane)

    def run(it, out, first, count):
        it.interpolate_device(d_frames.data_ptr() + first * fb, fb, d_frames.data_ptr() + (first + 1) * fb, fb, d_flows.data_ptr() + first * plane,
                              w, h, T, out.data_ptr() + first * fb, count, _stream())

    for mode in ("exact", "fma"):
        it = _interp(nsc, mode, ffmt, rounds)
        whole = guarded.full((N_PAIRS, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        halves = guarded.full((N_PAIRS, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        run(it, whole, 0, N_PAIRS)
        run(it, halves, 0, SPLIT), run(it, halves, SPLIT, N_PAIRS - SPLIT)
        got, want = fetch(whole), fetch(halves)
        bad = np.nonzero((got != want).reshape(N_PAIRS, -1).any(1))[0]
        assert bad.size == 0, (w, h, ffmt, rounds, mode, "pairs that differ from the two-call form", bad[:8], bad.size)
        if mode == "exact":
            for k in PROBES:
                assert np.array_equal(got[k], _oracle_frame(frames, seen, k, T, rounds)), (w, h, ffmt, rounds, k, "differs from the oracle")


@pytest.mark.parametrize("w,h", SPLIT_SIZES)
def test_multi_time_warp_across_the_launch_split(nsc, w, h):
    """nus_interp_interpolate_multi_device, 3 times, out_pair_stride with a gap: the only test in which launch_warp_blend advances
    the flow AND the output under a multi-time stride past the split.  The gaps keep their poison."""
    import torch

    frames, flows, _ = _split_content(w, h)
    times = [0.25, 0.5, float(np.float32(0.7))]
    fb, plane = w * h * 4, w * h * 8
    stride = 3 * fb + 16
    d_frames, d_flows = put(frames), put(flows)
    _assert_pair_form(w, h, d_frames.data_ptr(), d_flows.data_ptr(), fb, plane, stride)

    def run(it, out, first, count):
        it.interpolate_multi_device(d_frames.data_ptr() + first * fb, fb, d_frames.data_ptr() + (first + 1) * fb, fb,
                                    d_flows.data_ptr() + first * plane, w, h, times, out.data_ptr() + first * stride, stride, count, _stream())

    for mode in ("exact", "fma"):
        it = _interp(nsc, mode, "f32", 0)
        whole = guarded.full((N_PAIRS, stride), POISON, dtype=torch.uint8, device="cuda:0")
        halves = guarded.full((N_PAIRS, stride), POISON, dtype=torch.uint8, device="cuda:0")
        run(it, whole, 0, N_PAIRS)
        run(it, halves, 0, SPLIT), run(it, halves, SPLIT, N_PAIRS - SPLIT)
        got, want = fetch(whole), fetch(halves)
        assert (got[:, 3 * fb:] == POISON).all(), (w, h, mode, "a gap between the pairs' frames was written")
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (w, h, mode, "pairs that differ from the two-call form", bad[:8], bad.size)
        if mode == "exact":
            for k in PROBES:
                for i, t in enumerate(times):
                    assert np.array_equal(got[k, i * fb:(i + 1) * fb].reshape(h, w, 4), _oracle_frame(frames, flows, k, t, 0)), (w, h, k, i)


def _seam(num, den):
    """The last frame at or before the split that is an output of the stream: a call over the frames up to it and one over the frames
    from it on follow the whole stream's schedule (a later stream's schedule starts at a real frame), and neither crosses the
    split.  65 535 at 12/5; at 5/2, where 65 535 * 5 is odd, 65 534."""
    s = next(s for s in range(SPLIT, 0, -1) if (s * num) % den == 0)
    assert SPLIT - den < s <= SPLIT and N_PAIRS - s <= SPLIT
    return s


@pytest.mark.parametrize("kind,rounds", [("flow", 0), ("flow", 1), ("zero", 0)])
@pytest.mark.parametrize("num,den", [(5, 2), (12, 5)])
@pytest.mark.parametrize("w,h", SPLIT_SIZES)
def test_conversion_across_the_launch_split(nsc, w, h, num, den, kind, rounds):
    """nus_interp_retime_device over 66 001 frames: the only test in which launch_retime_warp (first_pair + done, the flow plane,
    the frames -- k_retime_flow, k_retime_flow_proj, k_retime_warp_tiny<kTinyDense / kTinyProjected>, k_retime_blend) and
    launch_retime_real (k_retime_real: first_pair + done of the second chunk) run a second launch.  The whole call against two
    calls that meet at the seam frame (_seam) and against the oracle at the probe pairs; the seam frame is the input frame, once."""
    import torch

    frames, flows, _ = _split_content(w, h)
    n = N_PAIRS + 1
    fb, plane = w * h * 4, w * h * 8
    d_frames = put(frames)
    d_flows = put(flows) if kind == "flow" else None
    p_flows = d_flows.data_ptr() if kind == "flow" else 0
    _assert_pair_form(w, h, d_frames.data_ptr(), p_flows, fb, plane)
    tbl = _retime.schedule_array(n, num, den)
    n_out = len(tbl)
    s = _seam(num, den)
    j0 = _retime.first_output(s, num, den)
    assert tuple(tbl[j0, :2]) == (s, 0) and tbl[j0 - 1, 1] != 0 and tbl[j0 + 1, 1] != 0
    assert _retime.count(s + 1, num, den) == j0 + 1 and j0 + _retime.count(n - s, num, den) == n_out

    def run(it, out, first, count, j):
        it.retime_device(d_frames.data_ptr() + first * fb, fb, count, p_flows + first * plane if p_flows else 0, w, h, num, den,
                         out.data_ptr() + j * fb, 0, _stream())

    for mode in ("exact", "fma") if kind == "flow" else ("exact",):
        it = _interp(nsc, mode, "f32", rounds)
        whole = guarded.full((n_out, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        halves = guarded.full((n_out, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        run(it, whole, 0, n, 0)
        run(it, halves, 0, s + 1, 0), run(it, halves, s, n - s, j0)
        got, want = fetch(whole), fetch(halves)
        bad = np.nonzero((got != want).reshape(n_out, -1).any(1))[0]
        assert bad.size == 0, (w, h, num, den, kind, rounds, mode, "outputs that differ from the two-call form", bad[:8], tbl[bad[:8]])
        assert np.array_equal(got[j0], frames[s]), "the real frame at the seam"
        assert not np.array_equal(got[j0 - 1], frames[s]) and not np.array_equal(got[j0 + 1], frames[s]), "the seam frame appears once"
        real = np.nonzero(tbl[:, 1] == 0)[0]  # every real-frame output of the stream, both sides of the split
        assert np.array_equal(got[real], frames[tbl[real, 0]]), (w, h, num, den, "a real-frame output is not the input frame")
        if mode == "exact":
            t_of = _retime.times_of(tbl)
            for k in PROBES:
                js = range(_retime.first_output(k, num, den), _retime.first_output(k + 1, num, den))
                assert len(js) > 0 or den > num
                for j in js:
                    assert int(tbl[j, 0]) == k
                    if tbl[j, 1] != 0:
                        want_j = _oracle_frame(frames, flows if kind == "flow" else None, k, t_of[j], rounds)
                        assert np.array_equal(got[j], want_j), (w, h, num, den, kind, rounds, k, j, "differs from the oracle")


@pytest.mark.parametrize("num,den", [(5, 2), (12, 5)])
@pytest.mark.parametrize("w,h", SPLIT_SIZES)
def test_cut_rule_across_the_launch_split(nsc, w, h, num, den):
    """nus_scene_apply_cuts_retime_device over 66 001 frames with random flags: the only test in which launch_scene_apply_retime
    advances `cut` and first_pair by `done`.  EVERY output against numpy, and the whole call against two calls that meet at the seam."""
    import torch

    frames, _, cut = _split_content(w, h)
    n = N_PAIRS + 1
    fb = w * h * 4
    d_frames, d_cut = put(frames), put(cut)
    s = _seam(num, den)
    j0 = _retime.first_output(s, num, den)
    n_out = _retime.count(n, num, den)
    for fmt in (0, 3):
        want = _cut_reference(frames, cut, num, den, fmt)
        whole = guarded.full((n_out, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        halves = guarded.full((n_out, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        _apply_cuts(nsc, d_frames.data_ptr(), fb, n, w, h, fmt, num, den, d_cut.data_ptr(), whole.data_ptr())
        _apply_cuts(nsc, d_frames.data_ptr(), fb, s + 1, w, h, fmt, num, den, d_cut.data_ptr(), halves.data_ptr())
        _apply_cuts(nsc, d_frames.data_ptr() + s * fb, fb, n - s, w, h, fmt, num, den, d_cut.data_ptr() + s, halves.data_ptr() + j0 * fb)
        got = fetch(whole)
        bad = np.nonzero((got != want).reshape(n_out, -1).any(1))[0]
        assert bad.size == 0, (w, h, num, den, fmt, "outputs that differ from the rule in numpy", bad[:8], bad.size)
        assert np.array_equal(fetch(halves), got), (w, h, num, den, fmt, "the two-call form differs")
