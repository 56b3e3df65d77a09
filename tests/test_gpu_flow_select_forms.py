"""Every form of the select warp's launcher (launch_warp_blend_select, nus_k_warp_select.hip) on the MI355X: what
tests/test_gpu_flow_select.py, which holds the rule at two large sizes and the smallest ones with everything packed and aligned,
never launches.

  form table     the 16 instantiations k_warp_blend_flow_sel<MODE, HALF, XV, RV, MT> ([fma][half][pair][mt]) and the two
                 k_warp_blend_flow_sel_tiny<MT>, each at the sizes where its tile can go wrong: a ragged last block of rows for each
                 rows-per-thread count, exact and one-over block widths, the smallest tile frames.
  fallbacks      the pair form refused on an even width by the output pointer (4 mod 8) and by out_pair_stride (4 mod 8).
  planes         flow planes that start off a 16-byte boundary (the pair form loads two vectors at once), input strides that
                 differ between A and B with poisoned gaps, the four input formats, the end times t = 0 and t = 1, seven times.
  launch split   66 000 pairs: both flow planes advance by the pairs already launched at the 65 535-pair split.

The reference is tests/_flow_select.py::select_f32, byte for byte in EXACT mode; FMA mode is held by contract_pixels with either
candidate, at the two sizes of tests/test_gpu_flow_select.py where the restatement's undecided share is known.  Every case asserts
the host-side conditions that select its kernel (_form restates them), so a later change of a size cannot move it to another
kernel unnoticed; the last test holds that every form was launched.  Every device output comes from conftest.guarded."""
import functools

import numpy as np
import pytest

import _flow_select as S
import test_gpu_flow_select as G  # its input generators, its cached restatements, its FMA margins
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

POISON = 0x6D
TIMES3 = G.TIMES3
TIMES7 = [0.0, 0.125, 0.25, 0.5, float(np.float32(0.7)), 0.875, 1.0]  # the most one call takes, both end times among them
# (66, 9): a pair per thread, one row each, blocks of 4 rows -- the last block has 1 row of 4 (9 = 2 * 4 + 1) ... and (65, 10): one
# pixel, two rows 4 apart, blocks of 8 rows -- the last block has rows 8, 9 and their partners 12, 13 beyond the frame.
PAIR_SIZES = [(66, 9), (128, 8), (2, 2)]  # 128: exactly one block of 64 pairs wide; 2 x 2: the smallest tile frame
ONE_SIZES = [(65, 10), (129, 8), (3, 2)]  # 129: one pixel over two blocks of 64
TINY_SIZES = [(1, 1), (5, 1), (1, 7)]

_SEEN = {}  # form -> the cases that launched it


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _form(mode, ffmt, w, h, n_times, out_ptr, out_stride):
    """The kernel launch_warp_blend_select picks, restated from its conditions: the tiny kernel where warp_corner_ok fails (below
    2 px either way; these frames are far from its 4 GiB and 24-bit limits), else kernels[fma][half][xv_ok][mt] with xv_ok = even
    width and the pair's 8-byte store aligned by the output pointer and the pair stride."""
    mt = n_times > 1
    if w < 2 or h < 2:
        return ("tiny", mt)
    pair = w % 2 == 0 and out_ptr % 8 == 0 and out_stride % 8 == 0
    return (mode == "fma", ffmt == "f16", pair, mt)


def _name(form):
    if form[0] == "tiny":
        return f"k_warp_blend_flow_sel_tiny<{'true' if form[1] else 'false'}>"
    fma, half, pair, mt = form
    return (f"k_warp_blend_flow_sel<{'kWarpFma' if fma else 'kWarpExact'}, {'true' if half else 'false'}, {2 if pair else 1}, "
            f"{1 if pair else 2}, {'true' if mt else 'false'}>")


def _launch(it, mode, ffmt, w, h, times, n, a, a_stride, b, b_stride, fwd, bwd, expect, out_off=0, gap_bytes=0, tag=None):
    """One call of nus_interp_interpolate_select_device into a poisoned guarded buffer -> (n, len(times), h, w, 4).  a, b, fwd, bwd:
    device addresses.  out_off: bytes the output starts behind the buffer's (256-byte aligned) start; gap_bytes: room behind every
    pair's frames (out_pair_stride).  expect: "pair", "one" or "tiny", held against _form.  Nothing but the frames is written."""
    import torch

    fb, k = w * h * 4, len(times)
    stride = k * fb + gap_bytes
    buf = guarded.full((out_off + n * stride + 8,), POISON, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    out = buf.data_ptr() + out_off
    form = _form(mode, ffmt, w, h, k, out, stride)
    assert ("tiny" if form[0] == "tiny" else "pair" if form[2] else "one") == expect, (tag, w, h, out_off, gap_bytes, form, expect)
    it.interpolate_select_device(a, a_stride, b, b_stride, fwd, bwd, w, h, times, out, stride if gap_bytes else 0, n, _stream())
    raw = fetch(buf)
    assert (raw[:out_off] == POISON).all() and (raw[out_off + n * stride:] == POISON).all(), (tag, "a byte outside the output was written")
    body = raw[out_off:out_off + n * stride].reshape(n, stride)
    assert (body[:, k * fb:] == POISON).all(), (tag, "a gap behind a pair's frames was written")
    _SEEN.setdefault(form, []).append(tag or (mode, ffmt, w, h, k))
    return body[:, :k * fb].reshape(n, k, h, w, 4)


def _expect(w, h):
    return "tiny" if min(w, h) < 2 else "pair" if w % 2 == 0 else "one"


class _Inputs:
    """The three pairs of a size on the device, packed: the sliding stream of four frames and the two flow fields in `ffmt`."""

    def __init__(self, w, h, ffmt):
        self.w, self.h, self.ffmt, self.fb = w, h, ffmt, w * h * 4
        self.frames = put(np.ascontiguousarray(G._frames(w, h)))
        self.fwd, self.bwd = G._device_flows(w, h, ffmt)
        assert all(t.data_ptr() % 16 == 0 for t in (self.frames, self.fwd, self.bwd))

    def run(self, it, mode, times, expect=None, **kw):
        p = self.frames.data_ptr()
        return _launch(it, mode, self.ffmt, self.w, self.h, times, 3, p, self.fb, p + self.fb, self.fb, self.fwd.data_ptr(),
                       self.bwd.data_ptr(), expect or _expect(self.w, self.h), **kw)


def _assert_restatement(got, w, h, ffmt, times, rounds, tag, bgra=False):
    for k, t in enumerate(times):
        G._assert_bytes(got[:, k], G._want(w, h, ffmt, t, rounds, bgra)[0], (tag, w, h, ffmt, rounds, t))


def _assert_fma_contract(got, w, h, ffmt, times, rounds, tag):
    """tests/test_gpu_flow_select.py::test_fma_pixels_meet_the_warp_contract_with_a_candidate, for one call: every pixel meets the
    warp contract with gF or gR, with the restatement's choice where the two errors differ by more than the FMA samples can move
    them, and the share of pixels within that margin is under the cap the restatement gives for these inputs."""
    frames = G._frames(w, h)
    F, R = (G._as_read(f, ffmt) for f in G._flows(w, h))
    for k, t in enumerate(times):
        _, back, eF, eR = G._want(w, h, ffmt, t, rounds)
        undecided = 0
        for i in range(3):
            gF, gR = S.candidates_f32(F[i], R[i], t, rounds)
            ok_f = S.contract_pixels(got[i, k], frames[i], frames[i + 1], gF, t, G.FMA_POSITION_ULPS)
            ok_r = S.contract_pixels(got[i, k], frames[i], frames[i + 1], gR, t, G.FMA_POSITION_ULPS)
            assert (ok_f | ok_r).all(), (tag, w, h, ffmt, rounds, t, i, int((~(ok_f | ok_r)).sum()), np.argwhere(~(ok_f | ok_r))[:4].tolist())
            decided = np.abs(eF[i] - eR[i]) > G.DECIDED_MARGIN
            ok_choice = np.where(back[i], ok_r, ok_f)
            assert ok_choice[decided].all(), (tag, w, h, ffmt, rounds, t, i, np.argwhere(decided & ~ok_choice)[:4].tolist())
            undecided += int((~decided).sum())
        assert undecided / (3 * w * h) <= G.UNDECIDED_CAP, (tag, w, h, ffmt, rounds, t, undecided)


# ---- 1. the form table ---------------------------------------------------------------------------------------------------------------
# form -> (mode, flow format, the sizes that reach it, the times).  The EXACT rows run the new sizes against the restatement; the
# FMA rows the two sizes of tests/test_gpu_flow_select.py (67 x 45 odd: one pixel per thread, 130 x 70 even: a pair) under the contract.
FORM_TABLE = {}
for _half, _ffmt in ((False, "f32"), (True, "f16")):
    for _mt, _times in ((False, [0.5]), (True, TIMES3)):
        FORM_TABLE[(False, _half, True, _mt)] = ("exact", _ffmt, PAIR_SIZES, _times)
        FORM_TABLE[(False, _half, False, _mt)] = ("exact", _ffmt, ONE_SIZES, _times)
        FORM_TABLE[(True, _half, True, _mt)] = ("fma", _ffmt, [(130, 70)], _times)
        FORM_TABLE[(True, _half, False, _mt)] = ("fma", _ffmt, [(67, 45)], _times)
FORM_TABLE[("tiny", False)] = ("exact", "f32", TINY_SIZES, [0.5])
FORM_TABLE[("tiny", True)] = ("exact", "f16", TINY_SIZES, TIMES3)
assert len(FORM_TABLE) == 18


@pytest.mark.parametrize("form", sorted(FORM_TABLE, key=str), ids=_name)
def test_form_table(nsc, form):
    mode, ffmt, sizes, times = FORM_TABLE[form]
    for w, h in sizes:
        inputs = _Inputs(w, h, ffmt)
        for rounds in (0, 3):
            it = G._interp(nsc, rounds, mode, ffmt)
            before = len(_SEEN.get(form, []))
            got = inputs.run(it, mode, times, tag=("form table", mode, ffmt, w, h, len(times), rounds))
            assert len(_SEEN[form]) == before + 1, (form, w, h, "the case took another form than its row's")
            if mode == "exact":
                _assert_restatement(got, w, h, ffmt, times, rounds, "form table")
            else:
                _assert_fma_contract(got, w, h, ffmt, times, rounds, "form table")


# ---- 2. the pair form refused on an even width ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("how", ["out-4-mod-8", "stride-4-mod-8"])
def test_even_width_falls_back_to_one_pixel_per_thread(nsc, how, ffmt):
    """xv_ok's second and third condition: the output pointer at 4 mod 8, and out_pair_stride at 4 mod 8 (a gap of 4 bytes behind
    the pair's frames, so every second pair's frames start at 4 mod 8).  The one-pixel form runs where the pair form would fit by
    the width; the bytes are the restatement's, the gap and the bytes around the output keep their poison."""
    w, h = 66, 9
    kw = {"out_off": 4} if how == "out-4-mod-8" else {"gap_bytes": 4}
    inputs = _Inputs(w, h, ffmt)
    for rounds in (0, 2):
        it = G._interp(nsc, rounds, "exact", ffmt)
        for times in ([0.5], TIMES3):
            got = inputs.run(it, "exact", times, expect="one", tag=(how, ffmt, rounds, len(times)), **kw)
            _assert_restatement(got, w, h, ffmt, times, rounds, how)
            assert np.array_equal(got, inputs.run(it, "exact", times, expect="pair", tag=(how, "aligned"))), (how, ffmt, rounds)
    # FMA mode on the even one of the two large sizes: kernels[1][half][0][mt] where the existing test launches kernels[1][half][1][mt]
    w, h = 130, 70
    got = _Inputs(w, h, ffmt).run(G._interp(nsc, 3, "fma", ffmt), "fma", [0.5], expect="one", tag=(how, ffmt, "fma"), **kw)
    _assert_fma_contract(got, w, h, ffmt, [0.5], 3, how)


# ---- 3. flow planes off 16 bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("shifted", ["both", "forward", "backward"])
@pytest.mark.parametrize("w,h", [(66, 9), (65, 10), (5, 1)])
def test_flow_planes_off_a_16_byte_boundary(nsc, w, h, shifted, ffmt):
    """The planes need their cell's alignment only (8 bytes f32, 4 bytes f16), and the pair form loads two cells at once: f32
    planes 8 bytes behind a 16-byte boundary, f16 planes 4 bytes behind one, both planes or either alone."""
    import torch

    off = 8 if ffmt == "f32" else 4
    inputs = _Inputs(w, h, ffmt)
    ptr = {}
    for name, plane in (("forward", inputs.fwd), ("backward", inputs.bwd)):
        if shifted in ("both", name):
            raw = plane.view(torch.uint8).reshape(-1)
            room = torch.full((raw.numel() + 32,), 0xE1, dtype=torch.uint8, device="cuda:0")
            assert room.data_ptr() % 16 == 0
            room[off:off + raw.numel()] = raw
            ptr[name] = (room.data_ptr() + off, room)
            assert ptr[name][0] % 16 == off
        else:
            ptr[name] = (plane.data_ptr(), plane)
    p = inputs.frames.data_ptr()
    for rounds in (0, 1):
        it = G._interp(nsc, rounds, "exact", ffmt)
        for times in ([0.5], TIMES3):
            got = _launch(it, "exact", ffmt, w, h, times, 3, p, inputs.fb, p + inputs.fb, inputs.fb, ptr["forward"][0], ptr["backward"][0],
                          _expect(w, h), tag=("planes off 16", shifted, ffmt, w, h, rounds))
            _assert_restatement(got, w, h, ffmt, times, rounds, ("planes off 16", shifted))


# ---- 4. input strides ---------------------------------------------------------------------------------------------------------------
def _strided(frames, gap, fill):
    n, fb = len(frames), frames[0].size
    buf = np.full((n, fb + gap), fill, np.uint8)
    buf[:, :fb] = frames.reshape(n, fb)
    return buf


@pytest.mark.parametrize("w,h", [(66, 9), (65, 10), (5, 1)])
def test_padded_input_strides_and_separate_arrays(nsc, w, h):
    """a_stride != b_stride with A and B in arrays of their own, and the sliding stream with a padded stride; poison in the gaps.
    The gaps are never read -- the result is the packed call's whatever the poison -- and the frames are inputs."""
    frames = G._frames(w, h)
    inputs = _Inputs(w, h, "f32")
    it = G._interp(nsc, 1, "exact", "f32")
    packed = inputs.run(it, "exact", TIMES3, tag=("strides", "packed", w, h))
    _assert_restatement(packed, w, h, "f32", TIMES3, 1, "packed")
    fb = inputs.fb
    for fill in (0xE1, 0x1E):
        host_a, host_b, host_s = _strided(frames[:3], 12, fill), _strided(frames[1:], 20, fill), _strided(frames, 8, fill)
        d_a, d_b, d_s = put(host_a), put(host_b), put(host_s)
        got = _launch(it, "exact", "f32", w, h, TIMES3, 3, d_a.data_ptr(), fb + 12, d_b.data_ptr(), fb + 20, inputs.fwd.data_ptr(),
                      inputs.bwd.data_ptr(), _expect(w, h), tag=("strides", "separate arrays", w, h))
        assert np.array_equal(got, packed), (w, h, hex(fill), "separate arrays with padded strides differ from the packed call")
        got = _launch(it, "exact", "f32", w, h, TIMES3, 3, d_s.data_ptr(), fb + 8, d_s.data_ptr() + fb + 8, fb + 8, inputs.fwd.data_ptr(),
                      inputs.bwd.data_ptr(), _expect(w, h), tag=("strides", "padded stream", w, h))
        assert np.array_equal(got, packed), (w, h, hex(fill), "the padded sliding stream differs from the packed call")
        for d, host in ((d_a, host_a), (d_b, host_b), (d_s, host_s)):
            assert np.array_equal(fetch(d), host), "an input was written"
    assert np.array_equal(fetch(inputs.frames), frames)


# ---- 5. the input formats -----------------------------------------------------------------------------------------------------------
def test_x_formats_write_the_colour_bytes_and_opaque_alpha(nsc):
    """rgbx / bgrx: the colour bytes of the rgba / bgra call, every alpha byte 255 (the input's alpha is undefined); alpha does not
    vote, so the restatement picks the same vector whatever the frames' alpha holds, and for all four formats."""
    w, h = 130, 70
    inputs = _Inputs(w, h, "f32")
    got = {fmt: inputs.run(G._interp(nsc, 1, "exact", "f32", fmt), "exact", TIMES3, tag=("format", fmt)) for fmt in ("rgba", "bgra", "rgbx", "bgrx")}
    _assert_restatement(got["rgba"], w, h, "f32", TIMES3, 1, "rgba")
    _assert_restatement(got["bgra"], w, h, "f32", TIMES3, 1, "bgra", bgra=True)
    for x, full in (("rgbx", "rgba"), ("bgrx", "bgra")):
        assert np.array_equal(got[x][..., :3], got[full][..., :3]), x
        assert (got[x][..., 3] == 255).all(), x
        assert not (got[full][..., 3] == 255).all()
    frames = G._frames(w, h)
    opaque = frames.copy()
    opaque[..., 3] = 255
    F, R = G._flows(w, h)
    for k, t in enumerate(TIMES3):
        back = G._want(w, h, "f32", t, 1)[1]
        assert np.array_equal(back, G._want(w, h, "f32", t, 1, True)[1])
        for i in range(3):
            frame_x, back_x, _, _ = S.select_f32(opaque[i], opaque[i + 1], F[i], R[i], t, 1)
            assert np.array_equal(back_x, back[i]), (t, i)
            assert np.array_equal(frame_x[..., :3], got["rgbx"][i, k][..., :3]), (t, i)


# ---- 6. FMA mode on tiny frames -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", TINY_SIZES)
def test_fma_mode_on_tiny_frames_is_exact(nsc, w, h, ffmt):
    """The tiny kernels are EXACT arithmetic in both modes: FMA mode writes the EXACT bytes, the restatement's."""
    inputs = _Inputs(w, h, ffmt)
    for rounds in (0, 3):
        for times in ([0.5], TIMES3):
            fma = inputs.run(G._interp(nsc, rounds, "fma", ffmt), "fma", times, tag=("tiny fma", w, h, ffmt, rounds))
            exact = inputs.run(G._interp(nsc, rounds, "exact", ffmt), "exact", times, tag=("tiny exact", w, h, ffmt, rounds))
            assert np.array_equal(fma, exact), (w, h, ffmt, rounds, len(times))
            _assert_restatement(fma, w, h, ffmt, times, rounds, "tiny fma")


# ---- 7. the end times and the full set ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", [(66, 9), (65, 10), (5, 1)])
def test_end_times_and_seven_times(nsc, w, h, ffmt):
    """t = 0 and t = 1: F is projected at t and R at 1 - t, so at an end time one of them is not projected at all while the other
    moves the whole way.  Seven times in one call: the most the time set holds.  Each frame is the single-time call's and the
    restatement's."""
    inputs = _Inputs(w, h, ffmt)
    for rounds in (0, 3):
        it = G._interp(nsc, rounds, "exact", ffmt)
        for times in ([0.0, 1.0], TIMES7):
            got = inputs.run(it, "exact", times, tag=("times", w, h, ffmt, rounds, len(times)))
            _assert_restatement(got, w, h, ffmt, times, rounds, "times")
            for k, t in enumerate(times):
                one = inputs.run(it, "exact", [t], tag=("times", "single", t))
                assert np.array_equal(one[:, 0], got[:, k]), (w, h, ffmt, rounds, t)


# ---- 8. no pair -----------------------------------------------------------------------------------------------------------------------
def test_no_pair_is_ok_and_writes_nothing(nsc):
    import torch

    w, h = 66, 9
    inputs = _Inputs(w, h, "f32")
    it = G._interp(nsc, 1, "exact", "f32")
    p = inputs.frames.data_ptr()
    for times in ([0.5], TIMES3):
        out = guarded.full((3, len(times), h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        it.interpolate_select_device(p, inputs.fb, p + inputs.fb, inputs.fb, inputs.fwd.data_ptr(), inputs.bwd.data_ptr(), w, h, times,
                                     out.data_ptr(), 0, 0, _stream())
        assert (fetch(out) == POISON).all()


# ---- 9. the launch split at 65 535 pairs ----------------------------------------------------------------------------------------------
N_PAIRS, SPLIT = 66000, 65535
PROBES = [0, 1, SPLIT - 1, SPLIT, SPLIT + 1, N_PAIRS - 1]
SPLIT_SIZES = [(4, 2), (3, 2), (2, 1)]  # the tile's pixel-pair form, its one-pixel form, the tiny kernels
T = float(np.float32(0.37))


@functools.lru_cache(maxsize=None)
def _split_content(w, h):
    """(frames (N_PAIRS + 1, h, w, 4), F, R (N_PAIRS, h, w, 2) f32), read-only and random throughout, F and R independently: an
    offset that forgets the pairs already launched, on either plane, cannot land on equal data."""
    rng = np.random.default_rng(6600 + 31 * w + h)
    frames = rng.integers(0, 256, (N_PAIRS + 1, h, w, 4), dtype=np.uint8)
    F = rng.uniform(-2.5, 2.5, (N_PAIRS, h, w, 2)).astype(np.float32)
    R = rng.uniform(-2.5, 2.5, (N_PAIRS, h, w, 2)).astype(np.float32)
    for a in (frames, F, R):
        a.setflags(write=False)
    return frames, F, R


@pytest.mark.parametrize("rounds", [0, 1])
@pytest.mark.parametrize("ffmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", SPLIT_SIZES)
def test_select_warp_across_the_launch_split(nsc, w, h, ffmt, rounds):
    """nus_interp_interpolate_select_device over 66 000 pairs: the only test in which the chunk lambda of launch_warp_blend_select
    runs a second launch and advances the frames, the output and BOTH flow planes by `done`.  The whole call against two calls
    that do not cross the split (65 535 + 465), in both modes; EXACT against the restatement at the pairs around the split."""
    import torch

    frames, F, R = _split_content(w, h)
    cast = (lambda f: f) if ffmt == "f32" else (lambda f: f.astype(np.float16))
    fb, plane = w * h * 4, w * h * (8 if ffmt == "f32" else 4)
    d_frames, d_fwd, d_bwd = put(frames), put(np.ascontiguousarray(cast(F))), put(np.ascontiguousarray(cast(R)))
    assert all(v % 16 == 0 for v in (d_frames.data_ptr(), d_fwd.data_ptr(), d_bwd.data_ptr()))

    def run(it, mode, out, first, count):
        form = _form(mode, ffmt, w, h, 1, out.data_ptr() + first * fb, fb)
        assert ("tiny" if form[0] == "tiny" else "pair" if form[2] else "one") == _expect(w, h), (w, h, first, form)
        it.interpolate_select_device(d_frames.data_ptr() + first * fb, fb, d_frames.data_ptr() + (first + 1) * fb, fb, d_fwd.data_ptr() + first * plane,
                                     d_bwd.data_ptr() + first * plane, w, h, [T], out.data_ptr() + first * fb, 0, count, _stream())
        _SEEN.setdefault(form, []).append(("launch split", mode, ffmt, w, h, rounds, first, count))

    for mode in ("exact", "fma"):
        it = G._interp(nsc, rounds, mode, ffmt)
        whole = guarded.full((N_PAIRS, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        halves = guarded.full((N_PAIRS, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")
        run(it, mode, whole, 0, N_PAIRS)
        run(it, mode, halves, 0, SPLIT), run(it, mode, halves, SPLIT, N_PAIRS - SPLIT)
        got, want = fetch(whole), fetch(halves)
        bad = np.nonzero((got != want).reshape(N_PAIRS, -1).any(1))[0]
        assert bad.size == 0, (w, h, ffmt, rounds, mode, "pairs that differ from the two-call form", bad[:8], bad.size)
        if mode == "exact":
            for k in PROBES:
                f, r = (cast(x[k]).astype(np.float32) for x in (F, R))
                assert np.array_equal(got[k], S.select_f32(frames[k], frames[k + 1], f, r, T, rounds)[0]), (w, h, ffmt, rounds, k, "differs from the restatement")


# ---- the census -----------------------------------------------------------------------------------------------------------------------
def test_every_select_form_was_launched():
    """Runs last: the 16 tile instantiations and the 2 tiny kernels, with how many launches of this module reached each."""
    print()
    for form in sorted(FORM_TABLE, key=str):
        cases = _SEEN.get(form, [])
        print(f"{_name(form):72s} {len(cases):3d} launches, first: {cases[0] if cases else '-'}")
    missing = [_name(f) for f in FORM_TABLE if f not in _SEEN]
    assert not missing, missing
    assert set(_SEEN) == set(FORM_TABLE), sorted(map(str, set(_SEEN) - set(FORM_TABLE)))
