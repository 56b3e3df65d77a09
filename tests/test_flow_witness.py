"""The C oracle of the optical-flow front end (oracle/nus_oracle.c, f32, the shaders' operation order) against an independent
float64 witness (tests/_flow64.py, vectorised numpy written from the shaders' definitions).  The HIP kernels are held to the
oracle bit for bit (tests/test_flow.py); a stencil, weight or sign the oracle had wrong would pass there.  It does not pass here.
CPU only.

Measured |oracle - witness| on the estimator cases below (x86-64, gcc -O2 -ffp-contract=off), worst case per content class:

    smooth pairs   1.74e-5 px   (130x17, 4 levels, 11 + 3 steps; flows up to 3 px)
    noise pairs    4.83e-5 px   (1920x1080, 3 levels, 50 + 10 steps; flows up to 16 px)

The tests assert 4 x these (7.0e-5 and 1.93e-4 px; the factor covers the summation order of another compiler or libm), both
under 2.5e-4 px, a quarter of FAST mode's 1e-3 px contract: the witness can referee that contract.  With the centre left out
of the 3x3 mean the disagreement is 2e-2 .. 1.1 px, with top-left instead of half-pixel upsampling 1e-2 .. 3.2 px (measured on
the small cases): two to four orders of magnitude beyond the bounds.  ESTIMATE_CASES is every (size, levels, steps) an
estimator test of tests/test_flow.py uses, the 1080p product configuration (3 levels, 50 + 10 + 10 steps) included; each runs
on a smooth pair and on a noise pair.
"""
import numpy as np
import pytest

import _flow64 as wit

U = 2.0 ** -24  # unit roundoff of f32: one rounding moves a value v by at most U * |v|
REFEREE = 2.5e-4  # a quarter of FAST mode's contract: no bound on |oracle - witness| asserted here may exceed it
BOUND = {"smooth": 4 * 1.74e-5, "noise": 4 * 4.83e-5}

# (w, h, levels, coarse steps, refine steps): the estimator cases of tests/test_flow.py, module order, duplicates dropped
ESTIMATE_CASES = [(192, 108, 3, 60, 15), (67, 35, 3, 11, 3), (130, 17, 4, 11, 3), (64, 16, 2, 11, 3), (33, 33, 6, 11, 3), (5, 3, 3, 11, 3),
                  (131, 203, 3, 11, 3), (249, 130, 2, 11, 3), (96, 50, 1, 9, 0), (96, 50, 1, 0, 0), (96, 50, 3, 0, 4), (96, 50, 3, 5, 0),
                  (96, 50, 2, 17, 9), (1037, 1029, 2, 4, 5), (613, 517, 2, 4, 5), (160, 90, 4, 30, 8), (97, 45, 3, 9, 3), (333, 262, 3, 7, 6),
                  (160, 96, 3, 20, 5), (613, 517, 2, 11, 5), (64, 64, 1, 13, 0), (129, 70, 2, 1, 1), (13, 9, 3, 5, 2), (9, 7, 3, 4, 2),
                  (5, 5, 2, 3, 1), (3, 33, 2, 3, 2), (1030, 5, 2, 2, 2), (1920, 1080, 3, 50, 10), (1920, 1080, 3, 10, 5), (129, 700, 2, 4, 3),
                  (160, 90, 2, 30, 8), (480, 270, 1, 50, 0), (333, 100, 1, 37, 0), (160, 96, 3, 20, 10), (333, 262, 3, 7, 7), (97, 45, 2, 9, 5),
                  (130, 70, 2, 4, 0), (1030, 6, 2, 2, 2), (2, 2, 1, 3, 0), (960, 540, 3, 10, 10), (480, 270, 3, 50, 10),
                  # sizes, levels and steps of the static-scene tests (here on the smooth and noise pairs)
                  (160, 120, 1, 64, 0), (160, 120, 2, 48, 40), (131, 70, 1, 64, 0), (131, 70, 2, 48, 40)]
LAMBDA = 0.02 ** 2


def _smooth(w, h, shift=0.0):
    """The smooth textured RGBA8 frame of tests/test_flow.py, content displaced by `shift` pixels in x."""
    x = np.arange(w, dtype=np.float64)[None, :] - shift
    y = np.arange(h, dtype=np.float64)[:, None]
    v = 127.5 + 45 * np.sin(x / 3.0) * np.cos(y / 4.0) + 50 * np.sin((x + 2 * y) / 23.0) + 25 * np.sin(x / 9.0 + y / 11.0)
    img = np.empty((h, w, 4), np.uint8)
    img[..., 0] = np.clip(v, 0, 255)
    img[..., 1] = np.clip(255 - v, 0, 255)
    img[..., 2] = np.clip(v * 0.5 + 40, 0, 255)
    img[..., 3] = 255
    return img


def _pair(oracle_mod, kind, w, h):
    if kind == "smooth":
        return _smooth(w, h, 0.0), _smooth(w, h, 1.3)
    return oracle_mod.gen_noise(w, h, 41), oracle_mod.gen_noise(w, h, 42)


def _maxdiff(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("size", [(65, 33), (1, 1), (5, 3), (130, 71)])
def test_oracle_primitives_match_the_float64_witness(oracle_mod, size):
    """Each bound is the operation count of the f32 form times the unit roundoff U = 2^-24 times the operand magnitude."""
    w, h = size
    u8 = oracle_mod.gen_noise(w, h, 31)
    img = oracle_mod.rgba8_to_f32(u8)
    # one correctly rounded division of a value <= 1
    assert _maxdiff(img, wit.to_float(u8)) <= U
    # per pass: one rounded product (the weights 1/16 and 4/16 are powers of two, 6/16 is not) and four rounded sums, all <= 1
    d = _maxdiff(oracle_mod.blur(img), wit.blur(img))
    print(f"blur {size}: {d:.2e}")
    assert d <= 10 * U
    # three sums of magnitude <= 2, 3, 4 (each rounding <= U * |sum|), then an exact * 0.25
    d = _maxdiff(oracle_mod.downsample(img), wit.downsample(img))
    print(f"downsample {size}: {d:.2e}")
    assert d <= 0.25 * 9 * U
    rng = np.random.default_rng(w + h)
    f0 = rng.standard_normal((h, w, 2)).astype(np.float32)
    for (dw, dh, sc) in ((2 * w, 2 * h, 2.0), (2 * w - 1, 2 * h - 1, 2.0), (w, h, 1.0), (3 * w + 1, h + 2, 0.5)):
        # The f32 sample coordinate (x + 0.5) / dw * sw - 0.5 carries three roundings of values <= sw: it is off by <= 3 U sw
        # texels (and likewise in y), which moves the bilinear sample by that times the largest step between neighbouring
        # texels; the interpolation itself adds ten roundings of values <= max |f|.  All times the scale.
        step_x = float(np.abs(np.diff(f0, axis=1)).max()) if w > 1 else 0.0
        step_y = float(np.abs(np.diff(f0, axis=0)).max()) if h > 1 else 0.0
        bound = sc * (3 * U * w * step_x + 3 * U * h * step_y + 10 * U * float(np.abs(f0).max()))
        d = _maxdiff(oracle_mod.flow_upsample(f0, dw, dh, sc), wit.upsample(f0, dw, dh, sc))
        print(f"upsample {size} -> {(dw, dh)}: {d:.2e} (bound {bound:.2e})")
        assert d <= bound
        if (dw, dh) == (w, h):
            # Equal size: wherever the f32 coordinate (i + 0.5) / n * n - 0.5 comes out as exactly i on both axes, the sample is the
            # texel itself with weights (1, 0), and the result is f * 1 * 1 * scale: no rounding at all.  (It does at 65x33, 1x1
            # and 5x3; at 130x71 some columns land 2^-17 beside the centre, and the bound above applies.)
            def centred(n):
                i = np.arange(n, dtype=np.float32)
                return bool(np.all((i + np.float32(0.5)) / np.float32(n) * np.float32(n) - np.float32(0.5) == i))
            if centred(w) and centred(h):
                assert d == 0.0
            else:
                assert size == (130, 71)


@pytest.mark.parametrize("size", [(65, 33), (5, 3), (130, 71)])
@pytest.mark.parametrize("steps", [1, 4, 15, 60])
def test_oracle_horn_schunck_matches_the_float64_witness(oracle_mod, size, steps):
    """Jacobi steps from a random start on noise (flows grow to ~15 px).  One f32 step rounds the 9-term mean (ten roundings of
    values <= F = max |flow|), the numerator Ix ua + Iy va + It (five roundings of values <= F + 1, on top of derivatives that
    are themselves rounded: <= 8 U (F + 1)) and the update; an error e of the numerator reaches the flow as e |Ix| / (lambda +
    Ix^2 + Iy^2) <= e / (2 sqrt(lambda)).  That is <= U (F + 1) (13 + 13 / (2 sqrt(lambda))) per step, and the step does not expand
    differences (a mean, then a projection), so the steps' errors add at worst.  From four steps on that sum is larger than
    what the witness has to resolve, and the bound is the referee's 2.5e-4 px."""
    w, h = size
    img = oracle_mod.rgba8_to_f32(oracle_mod.gen_noise(w, h, 31))
    img2 = oracle_mod.rgba8_to_f32(oracle_mod.gen_noise(w, h, 32))
    f0 = np.random.default_rng(w + h).standard_normal((h, w, 2)).astype(np.float32)
    want = wit.horn_schunck(img, img2, f0, steps, LAMBDA)
    got = oracle_mod.horn_schunck(img, img2, f0, iterations=steps, lam=LAMBDA)
    big = float(np.abs(want).max())
    bound = min(steps * U * (big + 1) * (13 + 13 / (2 * np.sqrt(LAMBDA))), REFEREE)
    d = _maxdiff(got, want)
    print(f"horn_schunck {size} x {steps}: {d:.2e} = {d / bound:.3f} of the bound {bound:.2e} (max |flow| {big:.1f})")
    assert d <= bound


@pytest.fixture(scope="module")
def estimates(oracle_mod):
    """(oracle flow, witness flow) per case and content class: computed once, read by the tests below."""
    out = {}
    for case in ESTIMATE_CASES:
        w, h, levels, coarse, refine = case
        for kind in ("smooth", "noise"):
            a, b = _pair(oracle_mod, kind, w, h)
            got = oracle_mod.flow_estimate(a, b, levels, coarse, refine, LAMBDA)
            want = wit.estimate(a, b, levels, coarse, refine, LAMBDA)
            got.setflags(write=False)
            want.setflags(write=False)
            out[case, kind] = (got, want)
    return out


@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_oracle_flow_estimate_matches_the_float64_witness(estimates, kind):
    assert BOUND[kind] <= REFEREE
    worst = 0.0
    for case in ESTIMATE_CASES:
        got, want = estimates[case, kind]
        assert got.shape == want.shape
        d = _maxdiff(got, want)
        worst = max(worst, d)
        assert d <= BOUND[kind], (case, kind, d)
    print(f"flow_estimate, {kind}: worst |oracle - witness| = {worst:.3e} px (bound {BOUND[kind]:.2e})")


@pytest.mark.parametrize("wrong", ["centre left out of the 3x3 mean", "top-left instead of half-pixel upsampling"])
def test_the_bounds_can_see_a_wrong_stencil(oracle_mod, estimates, wrong):
    """A witness with one definition changed must leave the oracle by orders of magnitude more than the bounds allow --
    otherwise agreement within them would prove nothing about the definitions."""
    kw = {"include_centre": False} if wrong.startswith("centre") else {"half_pixel": False}
    seen = 0
    for case in [(67, 35, 3, 11, 3), (96, 50, 2, 17, 9), (160, 90, 4, 30, 8), (96, 50, 1, 9, 0)]:
        w, h, levels, coarse, refine = case
        if "half_pixel" in kw and levels == 1:
            continue  # one level: nothing is upsampled
        for kind in ("smooth", "noise"):
            a, b = _pair(oracle_mod, kind, w, h)
            got = estimates[case, kind][0]
            d = _maxdiff(got, wit.estimate(a, b, levels, coarse, refine, LAMBDA, **kw))
            print(f"{wrong}: {case} {kind}: {d:.2e} px = {d / BOUND[kind]:.0f} x the bound")
            assert d >= 100 * BOUND[kind], (case, kind, d)
            seen += 1
    assert seen >= 6
