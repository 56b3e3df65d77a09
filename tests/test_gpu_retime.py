"""Frame-rate conversion by a rational ratio on the MI355X: the device table equals the host table, and every output of
nus_interp_retime_device is byte for byte the copy (r_j == 0) or the single-time nus_interp_interpolate_device call for pair k_j at
t_j (r_j != 0) that include/nuscaler_hip.h states -- the tiny, the one-pixel and the pixel-pair kernels, one and several blocks,
both modes, both flow formats and zero flow, RGBA and BGRA input, projection rounds, tight and gapped output.  Every device output
comes from conftest.guarded; a gapped output keeps its poison."""
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
SETTINGS = list(itertools.product(["exact", "fma"], ["rgba", "bgra"], [0, 2], [False, True]))  # mode, input, rounds, gapped
POISON = 0xC3


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


def _convert(it, d_frames, d_flows, n, w, h, num, den, gapped):
    """(outputs (n_out, h, w, 4), the gaps' bytes)"""
    import torch

    fb = w * h * 4
    n_out = _retime.count(n, num, den)
    stride = fb + 16 if gapped else fb
    out = guarded.full((n_out, stride), POISON, dtype=torch.uint8, device="cuda:0")
    it.retime_device(d_frames.data_ptr(), fb, n, d_flows.data_ptr() if d_flows is not None else 0, w, h, num, den, out.data_ptr(),
                     stride if gapped else 0, _stream())
    got = fetch(out)
    return got[:, :fb].reshape(n_out, h, w, 4), got[:, fb:]


def _reference(it, d_frames, d_flows, n, w, h, num, den, cell):
    """Output by output from the entry points the suite already holds to the oracle: the zero-flow call at t = 0 for a real frame,
    the single-time call of pair k_j at t_j else.  One guarded buffer, one download."""
    import torch

    fb = w * h * 4
    sched = _retime.schedule(n, num, den)
    ref = guarded.empty((len(sched), h, w, 4), dtype=torch.uint8, device="cuda:0")
    base = d_frames.data_ptr()
    for j, (k, r, t) in enumerate(sched):
        dst = ref.data_ptr() + j * fb
        if r == 0:  # (the last frame has no successor: A and B are the frame itself)
            it.interpolate_device(base + k * fb, fb, base + k * fb, fb, 0, w, h, 0.0, dst, 1, _stream())
        else:
            flow = d_flows.data_ptr() + k * w * h * cell if d_flows is not None else 0
            it.interpolate_device(base + k * fb, fb, base + (k + 1) * fb, fb, flow, w, h, float(t), dst, 1, _stream())
    return fetch(ref)


@pytest.mark.parametrize("num,den", RATIOS)
@pytest.mark.parametrize("n_frames", [2, 3, 6, 9, 700])
def test_device_table_equals_the_host_table(nsc, n_frames, num, den):
    import torch

    lib = nsc._capi.lib()
    want = _retime.as_array(_retime.schedule(n_frames, num, den))
    host = np.zeros_like(want)
    assert lib.nus_retime_schedule(n_frames, num, den, 0, len(want), host.ctypes.data) == 0
    dev = guarded.full((len(want), 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    assert lib.nus_retime_schedule_device(n_frames, num, den, dev.data_ptr(), _stream()) == 0, nsc._capi.last_error()
    got = fetch(dev).view(np.uint32)
    assert np.array_equal(host, want)
    assert np.array_equal(got, want), (n_frames, num, den, np.argwhere(got != want)[:4])


def _check_case(nsc, its, frames, d_frames, d_flows, cell, flow, w, h, num, den, n, setting):
    mode, fmt, rounds, gapped = setting
    key = (mode, fmt, rounds)
    if key not in its:
        it = its[key] = nsc.WgpuFrameInterpolator()
        it.set_mode(mode), it.set_input_format(fmt), it.set_flow_project(rounds)
        if flow != "zero":
            it.set_flow_format(flow)
    it = its[key]
    got, gaps = _convert(it, d_frames, d_flows, n, w, h, num, den, gapped)
    want = _reference(it, d_frames, d_flows, n, w, h, num, den, cell)
    assert got.shape == want.shape
    bad = [j for j in range(len(got)) if not np.array_equal(got[j], want[j])]
    assert not bad, (w, h, flow, num, den, n, mode, fmt, rounds, gapped, bad, _retime.schedule(n, num, den)[bad[0]])
    assert (gaps == POISON).all(), (w, h, flow, num, den, n, "a gap was written")
    if fmt == "rgba":  # a real frame is the input frame itself
        for j, (k, r, _) in enumerate(_retime.schedule(n, num, den)):
            if r == 0:
                assert np.array_equal(got[j], frames[k]), (j, k)


@pytest.mark.parametrize("flow", ["zero", "f32", "f16"])
def test_every_setting_crossed_with_every_ratio_and_length_at_6x4(nsc, flow):
    """The full cross -- 6 ratios x 3 lengths x 16 settings -- at the smallest size the pixel-pair tile takes; the other sizes
    (next test) walk the settings diagonally."""
    w, h = 6, 4
    n_max = max(N_FRAMES)
    frames = _frames(n_max, w, h, 5)
    d_frames = put(frames)
    d_flows, cell = None, 8
    if flow != "zero":
        f = _flows(n_max - 1, w, h, 6)
        d_flows, cell = put(f if flow == "f32" else f.astype(np.float16)), 8 if flow == "f32" else 4
    its = {}
    for (num, den), n, setting in itertools.product(RATIOS, N_FRAMES, SETTINGS):
        _check_case(nsc, its, frames, d_frames, d_flows, cell, flow, w, h, num, den, n, setting)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("flow", ["zero", "f32", "f16"])
def test_every_output_equals_the_copy_or_the_single_time_call(nsc, w, h, flow):
    """Every size with every ratio and length; of the 16 settings each (ratio, length) case takes two, chosen by two fixed walks
    (i % 16 and (5 i + 3) % 16), so that every setting meets every size and flow kind but NOT every ratio: the full cross is the
    6x4 test above."""
    n_max = max(N_FRAMES)
    frames = _frames(n_max, w, h, 5)
    d_frames = put(frames)
    d_flows, cell = None, 8
    if flow != "zero":
        f = _flows(n_max - 1, w, h, 6)
        d_flows, cell = put(f if flow == "f32" else f.astype(np.float16)), 8 if flow == "f32" else 4
    its = {}
    for i, ((num, den), n) in enumerate(itertools.product(RATIOS, N_FRAMES)):
        # every setting with every size and flow kind: 18 cases walk the 16 combinations; the second walk is shifted by one
        for setting in (SETTINGS[i % 16], SETTINGS[(5 * i + 3) % 16]):
            _check_case(nsc, its, frames, d_frames, d_flows, cell, flow, w, h, num, den, n, setting)


@pytest.mark.parametrize("w,h", [(6, 4), (131, 10), (1, 2)])
@pytest.mark.parametrize("m", [2, 3, 8])
def test_integer_ratio_equals_the_multi_time_entry_point_in_display_order(nsc, w, h, m):
    import torch

    n = 4
    fb = w * h * 4
    frames = _frames(n, w, h, 8)
    d_frames, d_flows = put(frames), put(_flows(n - 1, w, h, 9))
    for mode in ("exact", "fma"):
        it = nsc.WgpuFrameInterpolator()
        it.set_mode(mode)
        got, _ = _convert(it, d_frames, d_flows, n, w, h, m, 1, False)
        # display order: the real frame, then its pair's in-between frames; the multi-time call leaves the real frames' gaps alone
        disp = guarded.full(((n - 1) * m + 1, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        it.interpolate_multi_device(d_frames.data_ptr(), fb, d_frames.data_ptr() + fb, fb, d_flows.data_ptr(), w, h, nsc.frame_times(m),
                                    disp.data_ptr() + fb, m * fb, n - 1, _stream())
        want = fetch(disp)
        assert (want[::m] == POISON).all()
        want[::m] = frames
        assert np.array_equal(got, want), (w, h, m, mode)
