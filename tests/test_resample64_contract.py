"""The float64 FMA-mode yardstick (tests/_resample64.py) is fair and has teeth, without a GPU.

Fair: the f32 CPU oracle -- sums in another order than any kernel, f32::round at ties -- meets the contract for every filter
on the shapes of every resize kernel family and on noise, opaque noise, flat-alpha regions and gradients.  Teeth: a result
that truncates, carries a twentieth of an LSB of bias, has its weights scaled by 1 + 1e-5, read one input column from its
neighbour or swapped R and B is rejected; round-half-to-even at exact ties is accepted."""
import numpy as np
import pytest

from _resample64 import assert_fma_contract, check_fma, contract_eps, eps_rule, resample64

# the shapes of every resize kernel family, small: x2, x3, x4, x3/2, x4/3, the P/Q factors, any-scale up-scales (four and two
# outputs per lane), ragged and exact down-scales, mixed, and a 32-tap-window down-scale
SHAPES = [((64, 36), (128, 72)), ((52, 20), (104, 40)), ((36, 20), (108, 60)), ((32, 16), (128, 64)), ((64, 36), (96, 54)),
          ((48, 18), (64, 24)), ((32, 12), (40, 15)), ((40, 15), (48, 18)), ((36, 12), (60, 20)), ((32, 12), (80, 30)),
          ((32, 12), (112, 42)), ((40, 15), (56, 21)), ((35, 15), (56, 24)), ((40, 15), (72, 27)), ((50, 31), (127, 64)),
          ((60, 34), (85, 48)), ((37, 21), (74, 42)), ((64, 48), (32, 24)), ((90, 60), (30, 20)), ((103, 57), (41, 23)),
          ((70, 40), (99, 17)), ((150, 30), (30, 10)), ((7, 5), (7, 5))]


def _contents(oracle_mod, w, h, seed):
    noise = oracle_mod.gen_noise(w, h, seed)
    opaque = noise.copy()
    opaque[..., 3] = 255
    flat = noise.copy()
    flat[: h // 3, :, 3] = 0
    flat[h // 3: 2 * h // 3, :, 3] = 128
    flat[2 * h // 3:, :, 3] = 255
    flat[:, w // 2:, 3] = 17
    return {"noise": noise, "opaque": opaque, "flat_alpha": flat, "gradient": oracle_mod.gen_gradient(w, h, seed % 7)}


@pytest.mark.parametrize("filt", [0, 1, 2])
@pytest.mark.parametrize("dims", SHAPES)
def test_oracle_meets_the_contract(oracle_mod, filt, dims):
    (w, h), (ow, oh) = dims
    for name, img in _contents(oracle_mod, w, h, 31 + filt).items():
        check_fma(oracle_mod, oracle_mod.resize(img, ow, oh, filt), img, ow, oh, filt, (filt, dims, name))


def test_oracle_meets_the_contract_on_a_wide_noise_frame(oracle_mod):
    """The issue's measurement shape: 240x48 -> 720x144 Lanczos-3 on noise, a few hundred thousand samples."""
    img = oracle_mod.gen_noise(240, 48, 5)
    for filt in (0, 1, 2):
        st = check_fma(oracle_mod, oracle_mod.resize(img, 720, 144, filt), img, 720, 144, filt, filt)
        assert st["differ"] == 0 or st["worst_tie"] < 1e-4, st


def test_resample64_batches_and_identity(oracle_mod):
    img = oracle_mod.gen_noise(20, 11, 9)
    assert np.array_equal(resample64(oracle_mod, img, 20, 11, 0), img.astype(np.float64))
    frames = np.stack([img, img[::-1].copy()])
    got = np.stack([oracle_mod.resize(f, 30, 17, 1) for f in frames])
    check_fma(oracle_mod, got, frames, 30, 17, 1, "batch")
    with pytest.raises(AssertionError, match=r"frame, y, x, channel\), v, got: \[\(\(1, "):
        bad = got.copy()
        bad[1, 3, 4, 2] ^= 0x40
        check_fma(oracle_mod, bad, frames, 30, 17, 1, "batch")


def test_eps_rule():
    assert eps_rule(6, 6) == pytest.approx(1e-3)
    assert eps_rule(2, 2) == pytest.approx(1e-3)
    assert eps_rule(32, 32) == pytest.approx(1e-3 * 64 / 12)


def _round(c):
    return np.floor(np.clip(c, 0, 255) + 0.5).astype(np.uint8)


@pytest.fixture(scope="module")
def case(oracle_mod):
    w, h, ow, oh = 240, 48, 720, 144
    img = oracle_mod.gen_noise(w, h, 77)
    return img, ow, oh, resample64(oracle_mod, img, ow, oh, 0), contract_eps(oracle_mod, w, h, ow, oh, 0)


def test_exact_rounding_of_v_passes(case):
    img, ow, oh, v, eps = case
    st = assert_fma_contract(_round(v), v, eps, "exact")
    assert st["differ"] == 0 and st["samples"] == ow * oh * 4


@pytest.mark.parametrize("fault", ["floor", "bias_0.05", "weight_scale_1e-5", "r_b_swapped"])
def test_checker_rejects_faults(case, fault):
    img, ow, oh, v, eps = case
    got = {"floor": lambda: np.floor(np.clip(v, 0, 255)).astype(np.uint8),
           "bias_0.05": lambda: _round(v + 0.05),
           "weight_scale_1e-5": lambda: _round(v * (1 + 1e-5)),
           "r_b_swapped": lambda: _round(v[..., [2, 1, 0, 3]])}[fault]()
    with pytest.raises(AssertionError, match="FMA contract violated"):
        assert_fma_contract(got, v, eps, fault)


def test_checker_rejects_one_input_column_shifted(oracle_mod, case):
    img, ow, oh, v, eps = case
    moved = img.copy()
    moved[:, 100] = img[:, 101]
    with pytest.raises(AssertionError, match="FMA contract violated"):
        assert_fma_contract(_round(resample64(oracle_mod, moved, ow, oh, 0)), v, eps, "column 100 read from 101")


def test_round_half_to_even_at_ties_passes(oracle_mod):
    """Triangle at x2 has dyadic weights (1/4, 3/4): many samples land exactly on .5, where round-half-to-even (what the kernels'
    f32 -> u8 conversion does) and floor(c + 0.5) differ by one -- which the contract allows."""
    img = oracle_mod.gen_noise(64, 36, 3)
    v = resample64(oracle_mod, img, 128, 72, 2)
    even = np.rint(np.clip(v, 0, 255)).astype(np.uint8)
    assert (even != _round(v)).sum() > 100  # the case really has ties
    st = assert_fma_contract(even, v, contract_eps(oracle_mod, 64, 36, 128, 72, 2), "half-even")
    assert st["worst_tie"] == 0.0
    # ... but the other neighbour where there is no tie is not
    bad = even.copy()
    frac = np.abs(np.clip(v, 0, 255) - np.floor(np.clip(v, 0, 255)) - 0.5)
    i = np.unravel_index(np.argmax(frac > 0.1), v.shape)
    bad[i] = bad[i] + 1 if bad[i] < 255 else bad[i] - 1
    with pytest.raises(AssertionError, match="1 of"):
        assert_fma_contract(bad, v, 1e-3, "off-tie neighbour")
