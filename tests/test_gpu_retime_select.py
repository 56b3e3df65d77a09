"""Rate conversion with the select warp on the MI355X, warp level (nus_interp_retime_select_device): every in-between output
against the float32 restatement of the select rule (tests/_flow_select.py) at the schedule's time (tests/_retime.py) -- which share
no device code with the kernel --, against nus_interp_interpolate_select_device's single-time frame in both modes, gapped strides,
R = -F against the plain conversion, and the launch split at 65 535 pairs.

Every case asserts the host-side condition that selects its kernel form: k_retime_flow_sel_tiny below 2 pixels either way ("tiny"),
else k_retime_flow_sel<.., XV = 2, RV = kSelRV[1]> where the width is even and the output base and stride are multiples of 8 ("xv2"),
else <.., XV = 1, RV = kSelRV[0]> ("xv1").  The two tile forms own different numbers of rows per thread, so a grid built for the
wrong one leaves rows unwritten or runs off the frame: the odd heights, the poison fill and the guard bands of conftest.guarded,
from which every device output comes."""
import functools

import numpy as np
import pytest

import _flow_select as S
import _retime
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

POISON = 0x6D
N = 5
RATIOS = [(5, 2), (2, 5), (12, 5), (1, 1), (8, 1)]  # pairs with none, one and seven in-between outputs; all real frames
# (w, h, the kernel form with tight frames): the one-pixel form; the smallest tile frame; odd width and height, one pixel per thread
# and two rows per thread; a pair per thread, more than one block each way
SIZES = [(1, 1, "tiny"), (5, 1, "tiny"), (1, 7, "tiny"), (2, 2, "xv2"), (67, 45, "xv1"), (130, 70, "xv2")]


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
    """(F, R), each (N - 1, h, w, 2) float32 -- four different pairs of flows for the four pairs of frames: smooth +-12 px; a
    motion boundary with sub-pixel parts; vectors that leave the frame; an independent smooth field.  Every R is a smooth field of
    its own.  A kernel that reads pair 0's plane for pair 2 shows up as wrong bytes."""
    rng = np.random.default_rng(9001 + 31 * w + h)
    step = np.full((h, w, 2), (-3.25, 1.5), np.float32)
    step[h // 2:, w // 2:] = (7.5, -2.75)
    outside = ((rng.random((h, w, 2)) - 0.5) * 6).astype(np.float32)
    outside[::3, 1::2] += (2.0 * w + 0.5, -1.5 * h - 0.25)
    outside[1::3, ::2] -= (1.25 * w, -3.0 * h)
    F = np.stack([_smooth(rng, w, h), step, outside, _smooth(rng, w, h)])
    R = np.stack([_smooth(rng, w, h) for _ in range(N - 1)])
    F.setflags(write=False), R.setflags(write=False)
    return F, R


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    f = np.random.default_rng(9101 + 31 * w + h).integers(0, 256, (N, h, w, 4), dtype=np.uint8)  # uniform noise
    f.setflags(write=False)
    return f


def _as_read(flows, ffmt):
    return flows if ffmt == "f32" else flows.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _want(w, h, ffmt, k, t_bits, rounds):
    """The restatement's frame of pair k at the f32 time with those bits, from the flows as the warp reads them."""
    frames = _frames(w, h)
    F, R = (_as_read(f, ffmt) for f in _flows(w, h))
    t = np.array([t_bits], np.uint32).view(np.float32)[0]
    out = S.select_f32(np.ascontiguousarray(frames[k]), np.ascontiguousarray(frames[k + 1]), F[k], R[k], t, rounds)[0]
    out.setflags(write=False)
    return out


def _bits(t):
    return int(np.array([t], np.float32).view(np.uint32)[0])


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


def _form(w, h, out_ptr, out_stride):
    """launch_retime_warp's select branch: the one-pixel kernel where !warp_corner_ok (here: below 2 px either way); else
    kernels[fma][half][pair_ok], pair_ok as the other flow branches compute it."""
    if w < 2 or h < 2:
        return "tiny"
    return "xv2" if w % 2 == 0 and out_ptr % 8 == 0 and out_stride % 8 == 0 else "xv1"


def _convert(it, d_frames, frame_stride, d_fwd, d_bwd, w, h, num, den, form, out_gap=0, n=N):
    """-> (n_out, h, w, 4).  Asserts the kernel form; with out_gap, that the gaps between the output frames keep their poison."""
    import torch

    fb = w * h * 4
    n_out = _retime.count(n, num, den)
    out = guarded.full((n_out, fb + out_gap), POISON, dtype=torch.uint8, device="cuda:0")
    assert _form(w, h, out.data_ptr(), fb + out_gap) == form, (w, h, out_gap, form)
    it.retime_select_device(d_frames, frame_stride, n, d_fwd.data_ptr(), d_bwd.data_ptr(), w, h, num, den, out.data_ptr(),
                            fb + out_gap if out_gap else 0, _stream())
    raw = fetch(out)
    assert (raw[:, fb:] == POISON).all(), (w, h, num, den, out_gap, "an output gap was written")
    return raw[:, :fb].reshape(n_out, h, w, 4)


# ---- 1. EXACT: byte for byte the restatement at the schedule's times -------------------------------------------------------------------
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h,form", SIZES)
def test_exact_outputs_equal_the_restatement(nsc, w, h, form, ffmt):
    frames = _frames(w, h)
    d_frames = put(np.ascontiguousarray(frames))
    d_fwd, d_bwd = _device_flows(w, h, ffmt)
    between = 0
    for rounds in (0, 2):
        it = _interp(nsc, rounds, "exact", ffmt)
        for num, den in RATIOS:
            got = _convert(it, d_frames.data_ptr(), w * h * 4, d_fwd, d_bwd, w, h, num, den, form)
            sched = _retime.schedule(N, num, den)
            assert len(got) == len(sched)
            for j, (k, r, t) in enumerate(sched):
                tag = (w, h, ffmt, rounds, num, den, j, k, float(t))
                if r == 0:
                    _assert_bytes(got[j], frames[k], (tag, "a real-frame output is not the input frame"))
                else:
                    between += 1
                    _assert_bytes(got[j], _want(w, h, ffmt, k, _bits(t), rounds), (tag, "differs from the restatement"))
    # in-between outputs of five frames: 11 - 3 real at 5/2, 2 - 1 at 2/5, 10 - 1 at 12/5, none at 1/1, 33 - 5 at 8/1
    assert between == 2 * (8 + 1 + 9 + 0 + 28)
    assert np.array_equal(fetch(d_frames), frames)  # the frames are inputs


# ---- 2. both modes: byte for byte the select warp's single-time frame -----------------------------------------------------------------
def _single_time_frames(it, d_frames, d_fwd, d_bwd, w, h, num, den, plane):
    """{j: frame} for every in-between output j: nus_interp_interpolate_select_device for pair k_j at t_j, one call each."""
    import torch

    fb = w * h * 4
    sched = _retime.schedule(N, num, den)
    js = [j for j, (_, r, _) in enumerate(sched) if r != 0]
    if not js:
        return {}
    out = guarded.full((len(js), h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
    for i, j in enumerate(js):
        k, _, t = sched[j]
        a = d_frames.data_ptr() + k * fb
        it.interpolate_select_device(a, fb, a + fb, fb, d_fwd.data_ptr() + k * plane, d_bwd.data_ptr() + k * plane, w, h, [float(t)],
                                     out.data_ptr() + i * fb, 0, 1, _stream())
    got = fetch(out)
    return {j: got[i] for i, j in enumerate(js)}


@pytest.mark.parametrize("mode,ffmt,fmt", [("exact", "f32", "rgba"), ("fma", "f32", "rgba"), ("fma", "f16", "rgba"), ("exact", "f16", "rgba"),
                                           ("fma", "f32", "bgra")])
@pytest.mark.parametrize("w,h,form", SIZES)
def test_outputs_equal_the_single_time_select_warp(nsc, w, h, form, mode, ffmt, fmt):
    frames = _frames(w, h)
    d_frames = put(np.ascontiguousarray(frames))
    d_fwd, d_bwd = _device_flows(w, h, ffmt)
    plane = w * h * (8 if ffmt == "f32" else 4)
    it = _interp(nsc, 2, mode, ffmt, fmt)
    real = frames[..., [2, 1, 0, 3]] if fmt == "bgra" else frames
    for num, den in RATIOS:
        got = _convert(it, d_frames.data_ptr(), w * h * 4, d_fwd, d_bwd, w, h, num, den, form)
        want = _single_time_frames(it, d_frames, d_fwd, d_bwd, w, h, num, den, plane)
        for j, (k, r, t) in enumerate(_retime.schedule(N, num, den)):
            tag = (w, h, mode, ffmt, fmt, num, den, j, k, float(t))
            _assert_bytes(got[j], real[k] if r == 0 else want[j], tag)
    if fmt == "bgra" and min(w, h) >= 2:  # the selector does something: the RGBA handle writes other bytes
        other = _convert(_interp(nsc, 2, mode, ffmt), d_frames.data_ptr(), w * h * 4, d_fwd, d_bwd, w, h, 5, 2, form)
        assert not np.array_equal(other, _convert(it, d_frames.data_ptr(), w * h * 4, d_fwd, d_bwd, w, h, 5, 2, form))


# ---- 3. gapped frame_stride and out_frame_stride ------------------------------------------------------------------------------------
def _strided(frames, gap, fill):
    n = len(frames)
    fb = frames[0].size
    buf = np.full((n, fb + gap), fill, np.uint8)
    buf[:, :fb] = frames.reshape(n, fb)
    return buf


@pytest.mark.parametrize("mode", ["exact", "fma"])
@pytest.mark.parametrize("w,h,form", [(130, 70, "xv2"), (67, 45, "xv1"), (5, 1, "tiny")])
def test_gapped_input_and_output_strides(nsc, w, h, form, mode):
    """The bytes are the tight call's; poison in the input gaps is never read -- another poison changes no byte -- and the output
    gaps keep theirs.  On the even-width frame an output gap of 16 keeps the pair form; a gap of 4 makes the stride a multiple of 4
    but not of 8 and selects the one-pixel-per-thread tile where the pair form would fit (asserted in _convert)."""
    frames = _frames(w, h)
    fb = w * h * 4
    d_fwd, d_bwd = _device_flows(w, h, "f32")
    it = _interp(nsc, 1, mode)
    tight = put(np.ascontiguousarray(frames))
    in_gap = 20
    gapped = [put(_strided(frames, in_gap, fill)) for fill in (0xE1, 0x1E)]
    for num, den in [(5, 2), (12, 5)]:
        want = _convert(it, tight.data_ptr(), fb, d_fwd, d_bwd, w, h, num, den, form)
        for out_gap, gap_form in ((16, form), (4, "xv1" if form == "xv2" else form)):
            assert (fb + out_gap) % 4 == 0 and (form != "xv2" or ((fb + out_gap) % 8 == 0) == (out_gap == 16))
            got = [_convert(it, g.data_ptr(), fb + in_gap, d_fwd, d_bwd, w, h, num, den, gap_form, out_gap) for g in gapped]
            _assert_bytes(got[0], want, (w, h, mode, num, den, out_gap, "the gapped call differs from the tight one"))
            _assert_bytes(got[1], want, (w, h, mode, num, den, out_gap, "an input gap was read"))
    for g, fill in zip(gapped, (0xE1, 0x1E)):
        assert np.array_equal(fetch(g), _strided(frames, in_gap, fill)), "the input stream was written"


# ---- 4. R = -F, rounds 0: every pixel a tie, the plain conversion's bytes ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "fma"])
@pytest.mark.parametrize("w,h,form", [(130, 70, "xv2"), (67, 45, "xv1"), (5, 1, "tiny")])
def test_negated_forward_flow_is_the_plain_conversion(nsc, w, h, form, mode):
    import torch

    F = _flows(w, h)[0]
    fb = w * h * 4
    d_frames, d_fwd, d_bwd = put(np.ascontiguousarray(_frames(w, h))), put(np.ascontiguousarray(F)), put(np.ascontiguousarray(-F))
    it = _interp(nsc, 0, mode)
    for num, den in RATIOS:
        got = _convert(it, d_frames.data_ptr(), fb, d_fwd, d_bwd, w, h, num, den, form)
        want = guarded.full(got.shape, POISON, dtype=torch.uint8, device="cuda:0")
        it.retime_device(d_frames.data_ptr(), fb, N, d_fwd.data_ptr(), w, h, num, den, want.data_ptr(), 0, _stream())
        _assert_bytes(got, fetch(want), ("R = -F", w, h, mode, num, den))


# ---- 5. the launch split at 65 535 pairs ----------------------------------------------------------------------------------------------
N_PAIRS, SPLIT = 66000, 65535
PROBES = [0, 1, SPLIT - 1, SPLIT, SPLIT + 1, N_PAIRS - 1]


@functools.lru_cache(maxsize=None)
def _split_content():
    """(frames (N_PAIRS + 1, 2, 2, 4), F, R (N_PAIRS, 2, 2, 2) f32), read-only and random throughout: an offset that forgets the
    pairs already launched cannot land on equal data."""
    rng = np.random.default_rng(9500)
    frames = rng.integers(0, 256, (N_PAIRS + 1, 2, 2, 4), dtype=np.uint8)
    F = rng.uniform(-2.5, 2.5, (N_PAIRS, 2, 2, 2)).astype(np.float32)
    R = rng.uniform(-2.5, 2.5, (N_PAIRS, 2, 2, 2)).astype(np.float32)
    for a in (frames, F, R):
        a.setflags(write=False)
    return frames, F, R


def _seam(num, den):
    """The last frame at or before the split that is an output of the stream: a call over the frames up to it and one over the frames
    from it on follow the whole stream's schedule, and neither crosses the split."""
    s = next(s for s in range(SPLIT, 0, -1) if (s * num) % den == 0)
    assert SPLIT - den < s <= SPLIT and N_PAIRS - s <= SPLIT
    return s


@pytest.mark.parametrize("num,den", [(5, 2), (12, 5)])
def test_conversion_across_the_launch_split(nsc, num, den):
    """66 000 pairs of 2 x 2 pixels: the only test in which launch_retime_warp's select branch runs a second launch -- frames, BOTH
    flow planes and first_pair advanced by the pairs already launched.  One call against two calls that meet at the seam frame, and
    the probe pairs either side of the split against the restatement."""
    import torch

    w = h = 2
    frames, F, R = _split_content()
    n = N_PAIRS + 1
    fb, plane = w * h * 4, w * h * 8
    d_frames, d_fwd, d_bwd = put(frames), put(F), put(R)
    tbl = _retime.schedule_array(n, num, den)
    n_out = len(tbl)
    s = _seam(num, den)
    j0 = _retime.first_output(s, num, den)
    assert tuple(tbl[j0, :2]) == (s, 0)
    assert _retime.count(s + 1, num, den) == j0 + 1 and j0 + _retime.count(n - s, num, den) == n_out

    def run(it, out, first, count, j):
        it.retime_select_device(d_frames.data_ptr() + first * fb, fb, count, d_fwd.data_ptr() + first * plane, d_bwd.data_ptr() + first * plane,
                                w, h, num, den, out.data_ptr() + j * fb, 0, _stream())

    for mode in ("exact", "fma"):
        it = _interp(nsc, 1, mode)
        whole = guarded.full((n_out, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        halves = guarded.full((n_out, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        assert _form(w, h, whole.data_ptr(), fb) == "xv2" and (halves.data_ptr() + j0 * fb) % 8 == 0
        run(it, whole, 0, n, 0)
        run(it, halves, 0, s + 1, 0), run(it, halves, s, n - s, j0)
        got, want = fetch(whole), fetch(halves)
        bad = np.nonzero((got != want).reshape(n_out, -1).any(1))[0]
        assert bad.size == 0, (num, den, mode, "outputs that differ from the two-call form", bad[:8], tbl[bad[:8]])
        real = np.nonzero(tbl[:, 1] == 0)[0]  # every real-frame output of the stream, both sides of the split
        assert np.array_equal(got[real], frames[tbl[real, 0]]), (num, den, "a real-frame output is not the input frame")
        if mode == "exact":
            t_of = _retime.times_of(tbl)
            for k in PROBES:
                js = range(_retime.first_output(k, num, den), _retime.first_output(k + 1, num, den))
                assert len(js) > 0
                for j in js:
                    assert int(tbl[j, 0]) == k
                    if tbl[j, 1] != 0:
                        want_j = S.select_f32(frames[k], frames[k + 1], F[k], R[k], t_of[j], 1)[0]
                        _assert_bytes(got[j], want_j, (num, den, k, j, "differs from the restatement"))


# ---- 6. refusals leave the output alone ---------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(nsc):
    """(tests/test_retime_select_host.py has every refusal's status and text; here: the output of a refused call keeps its poison.)"""
    import torch

    w, h = 6, 4
    fb = w * h * 4
    d_frames = put(np.ascontiguousarray(_frames(w, h)[:3]))
    d_flow = put(np.zeros((2, h, w, 2), np.float32))
    out = guarded.full((8, fb), POISON, dtype=torch.uint8, device="cuda:0")
    it = _interp(nsc, 0)
    good = dict(d_frames=d_frames.data_ptr(), frame_stride=fb, n_frames=3, d_flows_fwd=d_flow.data_ptr(), d_flows_bwd=d_flow.data_ptr(),
                width=w, height=h, num=5, den=2, d_out=out.data_ptr(), out_frame_stride=0, stream=_stream())
    for kw in (dict(d_flows_fwd=0), dict(d_flows_bwd=0), dict(num=9, den=1), dict(num=0), dict(n_frames=1), dict(frame_stride=fb - 4),
               dict(out_frame_stride=fb + 2), dict(d_flows_bwd=d_flow.data_ptr() + 4), dict(d_out=out.data_ptr() + 2)):
        with pytest.raises(ValueError, match="^nus_interp_retime_select_device:"):
            it.retime_select_device(**dict(good, **kw))
    assert (fetch(out) == POISON).all()
    it.retime_select_device(**good)  # the good call writes the 6 frames of 3 frames at 5/2 and nothing behind them
    got = fetch(out)
    assert (got[:6] != POISON).any(axis=1).all() and (got[6:] == POISON).all()
