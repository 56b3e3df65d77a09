"""The float64 yardstick of the dense-flow warp (tests/_warp64.py) is fair and has teeth, without a GPU.

Fair: the f32 CPU oracle (every product and sum rounded separately: position_ulps = 1) and a numpy float32 emulation of the FMA
form of warp_blend_pixel (positions as one FMA, fma(b, f, a nf) lerps, the w - 2 / h - 2 corner rule: position_ulps = 1/2) both
meet the contract, on noise frames with Gaussian and smooth flows, far-outside vectors, a row of zero flow, a row of whole-pixel
flow, rows whose samples land in [w - 2, w - 1] x [h - 2, h - 1] including exactly (w - 1, h - 1), and f16-rounded fields, at
t = 0.5, 0.3 and 0.125 -- with at least 0.9 of the bytes decided on every case.  Teeth: eight faults of the emulation are
rejected with a message that names the sample, among them one that today's "within 1 LSB, fewer than 0.1 % different" accepts.
The FMA emulation lives in this file only."""
import functools

import numpy as np
import pytest

import _blockmatch as bmref
from _warp64 import ARITH_BAND, _ulp32, edge_flow, warp_contract, warp_samples64

TIMES = [0.5, 0.3, 0.125]
SHAPES = [(64, 48), (61, 7), (130, 33), (334, 117), (1920, 40)]  # the GPU file's kernels' shapes, and the widest coordinates
MIN_DECIDED = 0.9


# ---- the FMA form in numpy float32 ---------------------------------------------------------------------------------------

def _fma32(a, b, c):
    """round_f32(a b + c) with ONE rounding, for f32 operands: the product is exact in float64, the sum is rounded to odd in
    float64 (TwoSum gives its exact error), and rounding a 53-bit round-to-odd value to 24 bits equals rounding the real sum."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = np.atleast_1d(p + c)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    fix = (err != 0.0) & ((bits & 1) == 0)  # the neighbour on the side of the real sum has the odd mantissa
    bits = bits + np.where(fix, np.where((err > 0.0) == (s > 0.0), 1, -1), 0)
    return bits.view(np.float64).astype(np.float32).reshape(np.broadcast_shapes(p.shape, c.shape))


def _emu_sample(img, x, y, fault):
    """sample_corner<kWarpFma>: clamp, texel pair from min(floor, w - 2), fraction against THAT corner, three fused lerps, floor."""
    h, w = img.shape[:2]
    one = np.float32(1.0)
    x = np.clip(x, np.float32(0.0), np.float32(w - 1))
    y = np.clip(y, np.float32(0.0), np.float32(h - 1))
    xb, yb = np.minimum(x.astype(np.int64), w - 2), np.minimum(y.astype(np.int64), h - 2)
    if fault == "border_fraction":  # the fraction against floor(x) (0 at x = w - 1) while the pair still starts at w - 2
        xf, yf = x - np.floor(x), y - np.floor(y)
    else:
        xf, yf = x - xb.astype(np.float32), y - yb.astype(np.float32)
    nxf, nyf = one - xf, one - yf
    px = img.astype(np.float32)
    xf, yf, nxf, nyf = xf[..., None], yf[..., None], nxf[..., None], nyf[..., None]
    top = _fma32(px[yb, xb + 1], xf, px[yb, xb] * nxf)
    bottom = _fma32(px[yb + 1, xb + 1], xf, px[yb + 1, xb] * nxf)
    value = _fma32(bottom, yf, top * nyf)
    if fault == "round_nearest":
        return np.minimum(np.floor(value + np.float32(0.5)), np.float32(255.0))
    return np.floor(value)  # 0 <= value <= 255 (+ an ulp), as the kernel


def emu_fma_warp(a, b, flow, t, fault=None):
    """warp_blend_pixel<kWarpFma> over one frame pair in numpy float32; `fault` turns it into one of the mutants."""
    h, w = a.shape[:2]
    t32 = np.float32(t)
    nt32 = np.float32(1.0) - t32
    fx, fy = flow[..., 0].astype(np.float32), flow[..., 1].astype(np.float32)
    if fault == "flow_y_negated":
        fy = -fy
    xs = np.broadcast_to(np.arange(w, dtype=np.float32)[None, :], (h, w))
    ys = np.broadcast_to(np.arange(h, dtype=np.float32)[:, None], (h, w))
    ax, ay = _fma32(-t32, fx, xs), _fma32(-t32, fy, ys)
    bx, by = _fma32(nt32, fx, xs), _fma32(nt32, fy, ys)
    if fault == "position_bias":
        ax, ay, bx, by = (v + np.float32(1.0 / 256.0) for v in (ax, ay, bx, by))
    sa, sb = _emu_sample(a, ax, ay, fault), _emu_sample(b, bx, by, fault)
    if fault == "raised_samples":  # 0.08 % of the truncated samples one count too high
        rng = np.random.default_rng(5)
        for s in (sa, sb):
            s[(rng.random(s.shape) < 0.0008) & (s < 255.0)] += np.float32(1.0)
    if fault == "times_swapped":
        out = np.floor(t32 * sa + nt32 * sb)
    elif fault == "fused_blend":
        out = np.floor(_fma32(nt32, sa, t32 * sb))
    else:
        out = np.floor(nt32 * sa + t32 * sb)
    out = np.minimum(out, np.float32(255.0)).astype(np.uint8)
    return np.ascontiguousarray(out[..., [2, 1, 0, 3]]) if fault == "r_b_swapped" else out


def test_fma32_rounds_once():
    f = np.float32
    # real sums 2^-60 below / above a tie of f32: a float64 sum drops the 2^-60, lands on the tie and ties-to-even picks the other
    assert _fma32(f(2.0 ** -12 * (1 + 2.0 ** -18)), f(2.0 ** -12 * (1 - 2.0 ** -18)), f(1.0 + 2.0 ** -23))[()] == f(1.0 + 2.0 ** -23)
    assert _fma32(f(1.0 + 2.0 ** -12), f(1.0 + 2.0 ** -12), f(2.0 ** -60))[()] == f(1.0 + 2.0 ** -11 + 2.0 ** -23)
    rng = np.random.default_rng(1)
    a, b, c = (rng.standard_normal(10000).astype(np.float32) for _ in range(3))
    exact = np.array([float(x) * float(y) + float(z) for x, y, z in zip(a, b, c)])  # (rounded once to 53 bits: as good as exact here)
    assert (np.abs(_fma32(a, b, c).astype(np.float64) - exact) <= 0.5 * _ulp32(exact) * (1 + 1e-9)).all()


# ---- content -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _frames(w, h):
    rng = np.random.default_rng(4001 + 31 * w + h)
    a, b = (rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(2))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _flows(w, h, t):
    """name -> flow field (f32, or f16 for the rounded one) for one pair at time t."""
    gauss = edge_flow(1, w, h, t, 11)[0]
    return {"gauss": gauss, "smooth": edge_flow(1, w, h, t, 12, kind="smooth")[0], "gauss_f16": gauss.astype(np.float16)}


def _share(st, tag):
    share = st["decided"] / st["samples"]
    print(f"{tag}: samples {st['samples']}, decided {share:.4f}, differ from all-floor {st['differ_from_floor'] / st['samples']:.2e}")
    assert share >= MIN_DECIDED, (tag, share)
    return share


# ---- fair ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_oracle_meets_the_contract(oracle_mod, w, h, t):
    a, b = _frames(w, h)
    for name, flow in _flows(w, h, t).items():
        got = oracle_mod.warp_blend(a, b, flow.astype(np.float32), t)
        _share(warp_contract(got, a, b, flow, t, 1.0, ("oracle", w, h, t, name)), ("oracle", w, h, t, name))


@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_fma_emulation_meets_the_contract(w, h, t):
    a, b = _frames(w, h)
    for name, flow in _flows(w, h, t).items():
        got = emu_fma_warp(a, b, flow, t)
        _share(warp_contract(got, a, b, flow, t, 0.5, ("fma emulation", w, h, t, name)), ("fma emulation", w, h, t, name))


def test_far_vectors_on_a_small_frame_are_decided_by_the_integer_position_rule():
    """64 x 48 with Gaussian flows of 40 px: most samples clamp to a border on one axis, many on both.  Measured before the rule
    (the band applied to clamped samples too): 0.76 - 0.83 decided."""
    w, h = 64, 48
    a, b = _frames(w, h)
    for t in TIMES:
        flow = edge_flow(1, w, h, t, 13, sigma=40.0)[0]
        _share(warp_contract(emu_fma_warp(a, b, flow, t), a, b, flow, t, 0.5, ("sigma 40", t)), ("sigma 40", t))


def test_zero_flow_and_end_times_are_the_frames_and_fully_decided(oracle_mod):
    w, h = 61, 7
    a, b = _frames(w, h)
    flow = edge_flow(1, w, h, 0.5, 14)[0]
    st = warp_contract(oracle_mod.warp_blend(a, b, None, 0.3), a, b, None, 0.3, 0.5, "zero flow")
    assert st["decided"] == st["samples"] and st["differ_from_floor"] == 0
    for t, frame in ((0.0, a), (1.0, b)):  # the weight of the other frame is 0 and this one is sampled at the pixel itself
        st = warp_contract(frame, a, b, flow, t, 0.5, ("end", t))
        assert st["differ_from_floor"] == 0


def test_stacks_and_time_lists(oracle_mod):
    w, h, n = 34, 9, 3
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (n + 1, h, w, 4), dtype=np.uint8)
    flow = edge_flow(n, w, h, 0.5, 15)
    times = [0.25, 0.5, 0.75]
    got = np.stack([np.stack([oracle_mod.warp_blend(frames[i], frames[i + 1], flow[i], t) for t in times]) for i in range(n)])
    st = warp_contract(got, frames[:-1], frames[1:], flow, times, 1.0, "stack")
    assert st["samples"] == got.size and st["violations"] == 0
    assert warp_contract(got[:, 1], frames[:-1], frames[1:], flow, 0.5, 1.0, "stack, one time")["samples"] == got[:, 1].size
    assert warp_contract(got[2], frames[2], frames[3], flow[2], times, 1.0, "pair, times")["samples"] == got[2].size
    bad = got.copy()
    bad[2, 1, 5, 20, 3] ^= 0x40
    with pytest.raises(AssertionError, match=r"1 of \d+ bytes .* got: \[\(\(2, 1, 5, 20, 3\), "):
        warp_contract(bad, frames[:-1], frames[1:], flow, times, 1.0, "stack")
    assert warp_contract(bad, frames[:-1], frames[1:], flow, times, 1.0, "stack", raise_on_violation=False)["violations"] == 1
    st = warp_contract(bad, frames[:-1], frames[1:], flow, times, 1.0, "stack, RGB only", channels=(0, 1, 2))  # the bad byte is alpha
    assert st["samples"] == got.size // 4 * 3
    bad[0, 0, 1, 2, 2] ^= 0x40
    with pytest.raises(AssertionError, match=r"1 of \d+ bytes .* got: \[\(\(0, 0, 1, 2, 2\), "):
        warp_contract(bad, frames[:-1], frames[1:], flow, times, 1.0, "stack, RGB only", channels=(0, 1, 2))


def test_samples_and_band_arithmetic():
    img = np.zeros((2, 3, 4), np.uint8)
    img[0, :, 0] = (10, 20, 40)
    img[1, :, 0] = (110, 120, 140)
    s = warp_samples64(img, np.array([0.25, 1.5, 2.0, 7.0, -3.0]), np.array([0.0, 0.5, 1.0, 0.25, 9.0]))[:, 0]
    assert np.array_equal(s, [12.5, 80.0, 140.0, 65.0, 110.0])
    assert _ulp32(np.array([0.0, 1.0, 1.5, 1919.0, 0.75]))[1:].tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -13, 2.0 ** -24]
    assert _ulp32(np.array([0.0]))[0] == 0.0
    assert ARITH_BAND == 2.0 ** -14 > 2 * (3 * 2.0 ** -17 + 255 * 2.0 ** -25) > 2 * (2 * 2.0 ** -17 + 255 * 2.0 ** -25)


# ---- teeth ---------------------------------------------------------------------------------------------------------------

FAULTS = ["position_bias", "round_nearest", "raised_samples", "border_fraction", "times_swapped", "fused_blend", "flow_y_negated",
          "r_b_swapped"]


@pytest.mark.parametrize("w,h", [(130, 33), (1920, 40)])
@pytest.mark.parametrize("fault", FAULTS)
def test_contract_rejects_faults(fault, w, h):
    a, b = _frames(w, h)
    t = 0.3  # (at a dyadic t the blend's products are exact: swapped times at 0.5 and a fused blend are no faults there)
    flow = edge_flow(1, w, h, t, 11)[0]
    got = emu_fma_warp(a, b, flow, t, fault)
    assert not np.array_equal(got, emu_fma_warp(a, b, flow, t))
    with pytest.raises(AssertionError, match=r"warp contract violated .* got: \[\(\(0, 0, \d+, \d+, [0-3]\), \d") as e:
        warp_contract(got, a, b, flow, t, 0.5, fault)
    print(str(e.value)[:400])


@pytest.mark.parametrize("w,h", [(61, 7), (1920, 40)])
def test_a_few_raised_samples_pass_the_old_criterion_and_fail_the_contract(oracle_mod, w, h):
    """0.08 % of the truncated samples one count high: no byte more than 1 off the oracle and fewer than 0.1 % of them
    different (or fewer than 4000 bytes), which is all the suite asked of FMA mode before -- the contract counts them.  (On
    frames of a few thousand pixels the share of such a result scatters around 0.1 %: 0.07 - 0.15 % at 64 x 48, 256 x 4 and
    130 x 33 with this draw, so the old criterion caught it or not by chance; the two shapes here are the ones it lets through
    by construction -- the small-frame waiver -- and by size.)"""
    a, b = _frames(w, h)
    for t in (0.5, 0.3):
        flow = (np.random.default_rng(w * 7 + h).standard_normal((h, w, 2)) * 6).astype(np.float32)
        got = emu_fma_warp(a, b, flow, t, "raised_samples")
        d = np.abs(got.astype(np.int16) - oracle_mod.warp_blend(a, b, flow, t).astype(np.int16))
        assert d.max() <= 1 and ((d > 0).mean() < 1e-3 or d.size < 4000), (d.max(), (d > 0).mean())
        st = warp_contract(got, a, b, flow, t, 0.5, "raised", raise_on_violation=False)
        clean = warp_contract(emu_fma_warp(a, b, flow, t), a, b, flow, t, 0.5, "clean")
        print(f"{w} x {h}, t = {t}: old criterion passed with {(d > 0).mean():.3%} bytes different; contract: {st['violations']} violations")
        assert st["violations"] > 0 and clean["violations"] == 0


# ---- block vectors at dyadic times: nothing to round, so FMA is EXACT ------------------------------------------------------

@pytest.mark.parametrize("w,h,bs", [(33, 17, 8), (33, 17, 16), (33, 17, 32), (200, 72, 8), (200, 72, 16), (200, 72, 32)])
def test_integer_vectors_at_dyadic_times_leave_nothing_to_round(oracle_mod, w, h, bs):
    """Integer vectors and t = k / 8: every position, fraction, product and sum of the sample is exactly representable, so ex =
    ey = 0 and no rounding takes place in either form: the FMA emulation equals the oracle byte for byte (the GPU file asserts
    the same of the kernel)."""
    a, b = _frames(w, h)
    vec = np.random.default_rng(9001 + 131 * w + 17 * h + bs).integers(-24, 25, (-(-h // bs), -(-w // bs), 2)).astype(np.int16)
    flow = bmref.dense_flow(vec, w, h, bs)
    for t in (0.5, 0.25, 0.75, 0.125, 0.375, 0.875):
        want = oracle_mod.warp_blend(a, b, flow, t)
        assert np.array_equal(emu_fma_warp(a, b, flow, t), want), (w, h, bs, t)
        warp_contract(want, a, b, flow, t, 0.5, ("dyadic", w, h, bs, t))
