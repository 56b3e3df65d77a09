"""Frame-rate conversion by a rational ratio on the MI355X: the device table equals the host table, and every output of
nus_interp_retime_device is byte for byte the copy (r_j == 0) or the single-time nus_interp_interpolate_device call for pair k_j at
t_j (r_j != 0) that include/nuscaler_hip.h states -- the tiny, the one-pixel and the pixel-pair kernels, one and several blocks,
both modes, both flow formats and zero flow, RGBA and BGRA input, projection rounds, tight and gapped output, gapped input, and
bases and strides that are multiples of 4 only.  The table is held up to the bounds: terms of 4096, a million frames.  Every device
output comes from conftest.guarded; a gapped output keeps its poison.  (The kernel forms of the block-vector route, the cut rule and
the launch split: test_gpu_retime_forms.py.)"""
import itertools

import numpy as np
import pytest

import _retime
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 1), (1, 2), (5, 3), (6, 4), (130, 9), (131, 10)]
N_FRAMES = [2, 3, 6]
RATIOS = [(5, 2), (12, 5), (2, 5), (1, 1), (8, 1), (1001, 400)]
BOUND_RATIOS = [(4096, 4095), (4095, 4096), (4093, 512)]  # the terms' bound, either way round, and the ratio's bound with a large term
SETTINGS = list(itertools.product(["exact", "fma"], ["rgba", "bgra"], [0, 2], [False, True]))  # mode, input, rounds, gapped
POISON = 0xC3
IN_POISON = 0x99
# The stream's layout.  tight; outputs 16 bytes apart; INPUT frames 16 bytes apart; both strides fb + 4 with d_out at a 4-mod-8
# address and an f32 d_flows at an 8-mod-16 address: everything the header allows ("a multiple of 4") and no more.
FORMS = {"tight": (0, 0, 0), "out16": (0, 16, 0), "in16": (16, 0, 0), "both4": (4, 4, 4)}  # input gap, output gap, offset of d_out


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _frames(n, w, h, seed):
    return np.random.default_rng(seed + 31 * w + h).integers(0, 256, (n, h, w, 4), dtype=np.uint8)


def _flows(n, w, h, seed):
    """Random vectors within +-12 px, the right half one constant vector: a step boundary down the middle."""
    f = np.random.default_rng(seed + 7 * w + h).uniform(-12.0, 12.0, (n, h, w, 2)).astype(np.float32)
    f[:, :, w // 2:] = (9.5, -6.25)
    return f


class _Stream:
    """Frames (n, h, w, 4) and the pairs' flows (host f32 (n - 1, h, w, 2), or None) on the device in one form's layout: the
    frames `stride` bytes apart with IN_POISON between them, the flows in the format `flow` names ("zero", "f32", "f16"), an f32 field
    of the "both4" form 8 bytes behind a 16-byte boundary."""

    def __init__(self, frames, flows, flow, form):
        n, h, w = frames.shape[:3]
        self.fb = fb = w * h * 4
        self.stride = fb + FORMS[form][0]
        buf = np.full((n, self.stride), IN_POISON, np.uint8)
        buf[:, :fb] = frames.reshape(n, fb)
        self._frames = put(buf)
        self.frames = self._frames.data_ptr()
        self.cell, self.flows, self._flows = 8, 0, None
        if flow != "zero":
            f = np.ascontiguousarray(flows if flow == "f32" else flows.astype(np.float16))
            self.cell = f.itemsize * 2
            shift = 8 if (form == "both4" and flow == "f32") else 0
            raw = np.full((shift + f.nbytes,), IN_POISON, np.uint8)
            raw[shift:] = f.reshape(-1).view(np.uint8)
            self._flows = put(raw)
            assert self._flows.data_ptr() % 16 == 0
            self.flows = self._flows.data_ptr() + shift


def _convert(it, S, n, w, h, num, den, form):
    """(outputs (n_out, h, w, 4), the gaps' bytes)"""
    import torch

    fb = w * h * 4
    n_out = _retime.count(n, num, den)
    _, out_gap, off = FORMS[form]
    stride = fb + out_gap
    buf = guarded.full((n_out * stride + 2 * off,), POISON, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    it.retime_device(S.frames, S.stride, n, S.flows, w, h, num, den, buf.data_ptr() + off, stride if out_gap else 0, _stream())
    raw = fetch(buf)
    assert (raw[:off] == POISON).all() and (raw[len(raw) - off:] == POISON).all(), "a byte outside the output stream was written"
    got = raw[off:len(raw) - off].reshape(n_out, stride)
    return got[:, :fb].reshape(n_out, h, w, 4), got[:, fb:]


def _reference(it, S, n, w, h, num, den):
    """Output by output from the entry points the suite already holds to the oracle: the zero-flow call at t = 0 for a real frame,
    the single-time call of pair k_j at t_j else, on the stream's own frames and flows.  One guarded buffer, one download."""
    import torch

    fb = w * h * 4
    sched = _retime.schedule(n, num, den)
    ref = guarded.empty((len(sched), h, w, 4), dtype=torch.uint8, device="cuda:0")
    for j, (k, r, t) in enumerate(sched):
        dst = ref.data_ptr() + j * fb
        a = S.frames + k * S.stride
        if r == 0:  # (the last frame has no successor: A and B are the frame itself)
            it.interpolate_device(a, fb, a, fb, 0, w, h, 0.0, dst, 1, _stream())
        else:
            flow = S.flows + k * w * h * S.cell if S.flows else 0
            it.interpolate_device(a, fb, a + S.stride, fb, flow, w, h, float(t), dst, 1, _stream())
    return fetch(ref)


@pytest.mark.parametrize("num,den", RATIOS + BOUND_RATIOS)
@pytest.mark.parametrize("n_frames", [2, 3, 6, 9, 700, 4097, 1050000])
def test_device_table_equals_the_host_table(nsc, n_frames, num, den):
    """k_retime_table (retime_pair and retime_time as the kernels evaluate them) and nus_retime_schedule against the numpy
    restatement, up to the bounds: terms of 4096 and 4095, where all 4096 remainders of 4096/4095 go through __fdiv_rn, and
    1 050 000 frames, where pair * num (device) and j * den (host) pass 2^32 -- the only test in which a 32-bit product in
    retime_pair or retime_entry shows.  The table (up to 134 MB at ratio 8) comes down once."""
    import torch

    lib = nsc._capi.lib()
    want = _retime.schedule_array(n_frames, num, den)
    if n_frames <= 700:  # the vectorised restatement is the list's
        assert np.array_equal(want, _retime.as_array(_retime.schedule(n_frames, num, den)))
    n_out = len(want)
    assert n_out == _retime.count(n_frames, num, den) == lib.nus_retime_count(n_frames, num, den)
    if n_frames == 1050000 and max(_retime.reduce(num, den)) >= 4093:
        assert int(want[-1, 0]) * _retime.reduce(num, den)[0] >= 1 << 32  # (the case is what the docstring says it is)
    host = np.zeros_like(want)
    assert lib.nus_retime_schedule(n_frames, num, den, 0, n_out, host.ctypes.data) == 0
    dev = guarded.full((n_out, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    assert lib.nus_retime_schedule_device(n_frames, num, den, dev.data_ptr(), _stream()) == 0, nsc._capi.last_error()
    got = fetch(dev).view(np.uint32)
    assert np.array_equal(host, want), (n_frames, num, den, np.argwhere(host != want)[:4])
    assert np.array_equal(got, want), (n_frames, num, den, np.argwhere(got != want)[:4])
    # windows (first, count) of the host table: at the start, across j den = 2^32 where the stream reaches it, at the end
    span = min(64, n_out)
    across = (1 << 32) // _retime.reduce(num, den)[1]
    firsts = {0, n_out - span} | ({across - span // 2} if span // 2 <= across <= n_out - span else set())
    for first in sorted(firsts):
        part = np.full((span + 1, 4), 0xA5A5A5A5, np.uint32)
        assert lib.nus_retime_schedule(n_frames, num, den, first, span, part.ctypes.data) == 0, nsc._capi.last_error()
        assert np.array_equal(part[:span], want[first:first + span]) and (part[span] == 0xA5A5A5A5).all(), (n_frames, num, den, first)


def _interp(nsc, its, flow, mode, fmt, rounds):
    key = (mode, fmt, rounds)
    if key not in its:
        it = its[key] = nsc.WgpuFrameInterpolator()
        it.set_mode(mode), it.set_input_format(fmt), it.set_flow_project(rounds)
        if flow != "zero":
            it.set_flow_format(flow)
    return its[key]


def _check_case(nsc, its, frames, streams, flow, w, h, num, den, n, setting):
    """setting: (mode, input format, rounds, form); form False / True are "tight" / "out16".  -> the frames."""
    mode, fmt, rounds, form = setting
    form = {False: "tight", True: "out16"}.get(form, form)
    it = _interp(nsc, its, flow, mode, fmt, rounds)
    S = streams[form]
    got, gaps = _convert(it, S, n, w, h, num, den, form)
    want = _reference(it, S, n, w, h, num, den)
    assert got.shape == want.shape
    bad = [j for j in range(len(got)) if not np.array_equal(got[j], want[j])]
    assert not bad, (w, h, flow, num, den, n, mode, fmt, rounds, form, bad, _retime.schedule(n, num, den)[bad[0]])
    assert (gaps == POISON).all(), (w, h, flow, num, den, n, "a gap was written")
    if fmt == "rgba":  # a real frame is the input frame itself
        for j, (k, r, _) in enumerate(_retime.schedule(n, num, den)):
            if r == 0:
                assert np.array_equal(got[j], frames[k]), (j, k)
    return got


def _streams(frames, flow, w, h, seed, forms=("tight",)):
    """{form: _Stream} over `frames` and, unless flow is "zero", the _flows of the size; "out16" reads the tight stream."""
    f = _flows(len(frames) - 1, w, h, seed) if flow != "zero" else None
    s = {form: _Stream(frames, f, flow, form) for form in forms}
    if "tight" in s:
        s["out16"] = s["tight"]
    return s


@pytest.mark.parametrize("flow", ["zero", "f32", "f16"])
def test_every_setting_crossed_with_every_ratio_and_length_at_6x4(nsc, flow):
    """The full cross -- 6 ratios x 3 lengths x 16 settings -- at the smallest size the pixel-pair tile takes; the other sizes
    (next test) walk the settings diagonally."""
    w, h = 6, 4
    frames = _frames(max(N_FRAMES), w, h, 5)
    streams = _streams(frames, flow, w, h, 6)
    its = {}
    for (num, den), n, setting in itertools.product(RATIOS, N_FRAMES, SETTINGS):
        _check_case(nsc, its, frames, streams, flow, w, h, num, den, n, setting)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("flow", ["zero", "f32", "f16"])
def test_every_output_equals_the_copy_or_the_single_time_call(nsc, w, h, flow):
    """Every size with every ratio and length; of the 16 settings each (ratio, length) case takes two, chosen by two fixed walks
    (i % 16 and (5 i + 3) % 16), so that every setting meets every size and flow kind but NOT every ratio: the full cross is the
    6x4 test above."""
    frames = _frames(max(N_FRAMES), w, h, 5)
    streams = _streams(frames, flow, w, h, 6)
    its = {}
    for i, ((num, den), n) in enumerate(itertools.product(RATIOS, N_FRAMES)):
        # every setting with every size and flow kind: 18 cases walk the 16 combinations; the second walk is shifted by one
        for setting in (SETTINGS[i % 16], SETTINGS[(5 * i + 3) % 16]):
            _check_case(nsc, its, frames, streams, flow, w, h, num, den, n, setting)


@pytest.mark.parametrize("w,h", [(6, 4), (130, 9), (131, 10)])
@pytest.mark.parametrize("flow", ["zero", "f32", "f16"])
def test_input_stride_and_pointers_aligned_to_4_only(nsc, w, h, flow):
    """The only test that gives nus_interp_retime_device an input frame_stride above w*h*4 (b = a + frame_stride and the
    per-pair frame offsets of launch_retime_warp and launch_retime_real) and bases and strides that are multiples of 4 and no
    more: on the even-width sizes "both4" turns pair_ok off through d_out % 8 and out_frame_stride % 8 (k_retime_flow /
    k_retime_flow_proj <.., XV = 1> on a frame the pair form would take) and, where npx % 4 == 0, takes the scalar
    k_retime_blend<false> and k_retime_real<false> through stream_shape; its f32 flow sits at an 8-mod-16 address, which alone
    would turn xv_ok off.  "in16" keeps every 16-byte form and moves only the frames.  Each output is the single-time call on the
    same strided frames, "both4" writes the tight form's frames, and neither the output gaps nor the bytes around the stream are
    written.  Every (ratio, length) case takes both forms; mode, input format and rounds walk as in the size test."""
    frames = _frames(max(N_FRAMES), w, h, 5)
    streams = _streams(frames, flow, w, h, 6, forms=("tight", "in16", "both4"))
    fb = w * h * 4
    # what selects the kernels, from the host side of launch_retime_warp and stream_shape
    S4 = streams["both4"]
    assert S4.stride == fb + 4 and S4.stride % 8 == 4 and streams["in16"].stride % 16 == fb % 16
    assert flow != "f32" or S4.flows % 16 == 8
    its = {}
    for i, ((num, den), n) in enumerate(itertools.product(RATIOS, N_FRAMES)):
        mode, fmt, rounds, _ = SETTINGS[(2 * i) % 16]  # (the form bit is dropped: 18 cases walk the 8 other combinations)
        tight = _check_case(nsc, its, frames, streams, flow, w, h, num, den, n, (mode, fmt, rounds, "tight"))
        for form in ("in16", "both4"):
            got = _check_case(nsc, its, frames, streams, flow, w, h, num, den, n, (mode, fmt, rounds, form))
            assert np.array_equal(got, tight), (w, h, flow, num, den, n, mode, fmt, rounds, form, "differs from the tight form")


@pytest.mark.parametrize("w,h", [(6, 4), (131, 10), (1, 2)])
@pytest.mark.parametrize("m", [2, 3, 8])
def test_integer_ratio_equals_the_multi_time_entry_point_in_display_order(nsc, w, h, m):
    import torch

    n = 4
    fb = w * h * 4
    frames = _frames(n, w, h, 8)
    flows = _flows(n - 1, w, h, 9)
    S = _Stream(frames, flows, "f32", "tight")
    d_frames, d_flows = put(frames), put(flows)
    for mode in ("exact", "fma"):
        it = nsc.WgpuFrameInterpolator()
        it.set_mode(mode)
        got, _ = _convert(it, S, n, w, h, m, 1, "tight")
        # display order: the real frame, then its pair's in-between frames; the multi-time call leaves the real frames' gaps alone
        disp = guarded.full(((n - 1) * m + 1, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        it.interpolate_multi_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_flows.data_ptr(), w, h, nsc.frame_times(m),
                                    disp.data_ptr() + fb, m * fb, n - 1, _stream())
        want = fetch(disp)
        assert (want[::m] == POISON).all()
        want[::m] = frames
        assert np.array_equal(got, want), (w, h, m, mode)
