"""GPU: every resize kernel family in FMA mode (the default) against the float64 contract of tests/_resample64.py.

Each output sample equals floor(c + 0.5) of the float64 resample from the oracle's tap weights, or its other neighbour within
eps of a rounding tie -- independent of the order of the kernel's sums, unlike "within 1 LSB of the oracle".  All three
filters; every case asserts its kernel_variant; content: noise, opaque noise (the 3-channel paths), flat-alpha regions and a
gradient, as the first, middle and last frames of one device batch; BGRA input; the fused blend -> upscale; both 4K outputs of
the one-launch unit step; one full 1080p -> 4K frame.  The last test asserts that every resize variant was seen and prints,
per kernel and filter, the fraction of samples that differ from floor(c + 0.5) and the worst tie distance among them."""
import numpy as np
import pytest

from _resample64 import assert_fma_contract, check_fma, contract_eps, resample64
from conftest import guarded  # device outputs between poisoned guard bands (tests/conftest.py)
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch  # host <-> HBM through nus_upload / nus_download

pytestmark = pytest.mark.gpu

RESIZE_VARIANTS = {"lanczos3_x2_regwin", "lanczos3_xs_regwin", "lanczos3_r32_regwin", "lanczos3_r43_regwin", "lanczos3_pq_regwin",
                   "resize_regwin_lds", "resize_rows_lds", "resize_down_stream", "lanczos3_general"}
FILTERS = [("lanczos3", 0), ("bicubic", 1), ("triangle", 2)]
_STATS = {}  # (kernel_variant, alg) -> [samples, differing samples, worst tie distance among them]


def _record(variant, alg, st):
    s = _STATS.setdefault((variant, alg), [0, 0, 0.0])
    s[0] += st["samples"]
    s[1] += st["differ"]
    if st["worst_tie"] is not None:
        s[2] = max(s[2], st["worst_tie"])


def _contents(oracle_mod, w, h, seed):
    """noise, opaque noise, flat-alpha regions (0 / 128 / 255 by rows, 17 over the right half), gradient."""
    noise = oracle_mod.gen_noise(w, h, seed)
    opaque = oracle_mod.gen_noise(w, h, seed + 1)
    opaque[..., 3] = 255
    flat = oracle_mod.gen_noise(w, h, seed + 2)
    flat[: h // 3, :, 3] = 0
    flat[h // 3: 2 * h // 3, :, 3] = 128
    flat[2 * h // 3:, :, 3] = 255
    flat[:, w // 2:, 3] = 17
    return {"noise": noise, "opaque": opaque, "flat_alpha": flat, "gradient": oracle_mod.gen_gradient(w, h, seed % 5)}


def _bgra(img):
    return np.ascontiguousarray(img[..., [2, 1, 0, 3]])


def _upscaler(nsc, alg, w, h, ow, oh, options, fmt="rgba"):
    u = nsc.PyWgpuUpscaler("quality", alg)
    for k, v in options.items():
        u.set_option(k, v)
    u.set_input_format(fmt)
    u.initialize(w, h, ow, oh)
    return u


def _device_batch(torch, u, frames_np, ow, oh):
    n = frames_np.shape[0]
    d_in = put(frames_np)
    d_out = guarded.empty((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
    u.upscale_device(d_in.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return fetch(d_out)


# (input size, output size, options, kernel variant), per family.  Strips of the x2 kernel are 240 input columns wide: 520 and
# 964 leave a ragged last strip, 90 / 45 rows a ragged last row block at every rows_per_wave.
CASES = {
    "x2": [((520, 90), (1040, 180), {}, "lanczos3_x2_regwin"),
           ((520, 90), (1040, 180), {"rows_per_wave": 7}, "lanczos3_x2_regwin"),
           ((964, 45), (1928, 90), {"rows_per_wave": 26}, "lanczos3_x2_regwin"),
           ((248, 40), (496, 80), {"rows_per_wave": 1}, "lanczos3_x2_regwin")],
    # x3: at 16 / 20 columns the interior weights are one set per phase; from 32 up they move with the binade of the coordinate
    # and the kernel takes them by weight class.  x4: one set per phase.
    "xs": [((16, 16), (48, 48), {}, "lanczos3_xs_regwin"), ((20, 20), (60, 60), {}, "lanczos3_xs_regwin"),
           ((64, 36), (192, 108), {}, "lanczos3_xs_regwin"), ((500, 19), (1500, 57), {"rows_per_wave": 7}, "lanczos3_xs_regwin"),
           ((64, 36), (256, 144), {}, "lanczos3_xs_regwin"), ((252, 20), (1008, 80), {}, "lanczos3_xs_regwin")],
    "r32": [((64, 36), (96, 54), {}, "lanczos3_r32_regwin"), ((1000, 50), (1500, 75), {"rows_per_wave": 6}, "lanczos3_r32_regwin"),
            ((744, 22), (1116, 33), {}, "lanczos3_r32_regwin")],
    "r43": [((48, 18), (64, 24), {}, "lanczos3_r43_regwin"), ((372, 33), (496, 44), {"rows_per_wave": 7}, "lanczos3_r43_regwin"),
            ((1116, 30), (1488, 40), {}, "lanczos3_r43_regwin")],
    "pq": [((64, 36), (80, 45), {}, "lanczos3_pq_regwin"), ((320, 25), (384, 30), {}, "lanczos3_pq_regwin"),
           ((372, 18), (620, 30), {}, "lanczos3_pq_regwin"), ((240, 30), (600, 75), {}, "lanczos3_pq_regwin"),
           ((248, 30), (868, 105), {}, "lanczos3_pq_regwin"), ((300, 20), (420, 28), {}, "lanczos3_pq_regwin"),
           ((315, 25), (504, 40), {}, "lanczos3_pq_regwin"), ((300, 20), (540, 36), {"rows_per_wave": 7}, "lanczos3_pq_regwin")],
    # four output columns per lane at x4 and x10, two at x1.4 and x1.006 (widest_footprint / widest_union in nus_plan.cpp)
    "regwin_lds": [((250, 135), (1000, 540), {}, "resize_regwin_lds"), ((100, 37), (1000, 99), {}, "resize_regwin_lds"),
                   ((480, 270), (680, 384), {}, "resize_regwin_lds"), ((517, 40), (520, 41), {}, "resize_regwin_lds")],
    "rows_lds": [((50, 31), (127, 64), {}, "resize_rows_lds"), ((97, 13), (101, 29), {}, "resize_rows_lds"),
                 ((320, 180), (480, 270), {"force_general": 1, "force_rows": 1}, "resize_rows_lds"),
                 ((300, 157), (150, 78), {"force_rows": 1}, "resize_rows_lds")],
    "down": [((300, 157), (150, 78), {}, "resize_down_stream"), ((515, 90), (172, 30), {}, "resize_down_stream"),
             ((464, 64), (232, 32), {"down_seg_width": 41}, "resize_down_stream"),
             ((700, 90), (233, 30), {"down_seg_width": 57}, "resize_down_stream"), ((130, 71), (129, 70), {}, "resize_down_stream"),
             ((64, 900), (16, 300), {}, "resize_down_stream")],
    "general": [((97, 13), (101, 29), {"force_general": 1, "force_per_pixel": 1}, "lanczos3_general"),
                ((100, 40), (30, 12), {"force_per_pixel": 1}, "lanczos3_general")],
}
_P_Q = {(80, 64): (5, 4), (384, 320): (6, 5), (620, 372): (5, 3), (600, 240): (5, 2), (868, 248): (7, 2), (420, 300): (7, 5),
        (504, 315): (8, 5), (540, 300): (9, 5)}


@pytest.mark.parametrize("alg,filt", FILTERS)
@pytest.mark.parametrize("family", list(CASES))
def test_resize_family_meets_fma_contract(nsc, oracle_mod, alg, filt, family):
    import torch

    for k, ((w, h), (ow, oh), opts, variant) in enumerate(CASES[family]):
        cont = _contents(oracle_mod, w, h, 500 + 10 * k + filt)
        frames = np.stack(list(cont.values()))
        batch = (w * h) % 4 == 0 and (ow * oh) % 4 == 0  # batched device frames are whole multiples of 16 bytes
        for fmt in ("rgba", "bgra") if k == 0 else ("rgba",):  # BGRA input: the first case of every family and filter
            u = _upscaler(nsc, alg, w, h, ow, oh, opts, fmt)
            assert u.kernel_variant == variant, (family, alg, (w, h), (ow, oh), opts, u.kernel_variant)
            if variant == "lanczos3_pq_regwin":
                assert (u.get_option("pq_p"), u.get_option("pq_q")) == _P_Q[(ow, w)]
                assert u.get_option("pq_narrow_active") == (0 if alg == "lanczos3" else 1)  # the 4-tap form of support <= 2
            if variant == "resize_regwin_lds":
                assert u.get_option("win_outputs_per_lane") == (4 if ow >= 2 * w else 2), (w, ow)
            src = frames if fmt == "rgba" else np.stack([_bgra(f) for f in frames])
            if batch:
                got = _device_batch(torch, u, src, ow, oh)
            else:
                got = np.stack([_device_batch(torch, u, f[None], ow, oh)[0] for f in src])
            for i, name in enumerate(cont):
                tag = (family, alg, (w, h), (ow, oh), opts, variant, fmt, name, f"frame {i} of {len(cont) if batch else 1}")
                _record(variant, alg, check_fma(oracle_mod, got[i], frames[i], ow, oh, filt, tag))


@pytest.mark.parametrize("alg,filt", FILTERS)
def test_fused_blend_upscale_meets_fma_contract(nsc, oracle_mod, alg, filt):
    """upscale_blend_device: the float64 reference is the resample of the oracle's bit-exact warp_blend (zero flow)."""
    import torch

    w, h, n = 248, 40, 4
    for t in (0.5, 0.3):
        frames_np = np.stack([oracle_mod.gen_noise(w, h, 300 + i) for i in range(n + 1)])
        frames_np[2, :, :, 3] = 255
        frames_np[3, : h // 2, :, 3] = 128
        frames = put(frames_np)
        u = _upscaler(nsc, alg, w, h, 2 * w, 2 * h, {})
        assert u.kernel_variant == "lanczos3_x2_regwin"
        out = guarded.empty((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device="cuda")
        fb = w * h * 4
        u.upscale_blend_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, t, out.data_ptr(), n,
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = fetch(out)
        for i in range(n):
            mid = oracle_mod.warp_blend(frames_np[i], frames_np[i + 1], None, t)
            _record("lanczos3_x2_regwin", alg, check_fma(oracle_mod, got[i], mid, 2 * w, 2 * h, filt, ("blend", alg, t, i)))


@pytest.mark.parametrize("alg,filt", FILTERS)
def test_unit_step_both_outputs_meet_fma_contract(nsc, oracle_mod, alg, filt):
    """upscale_unit_device: upscale(A) and upscale(blend(A, B)) of every unit; ragged last strip and row block."""
    import torch

    w, h, n, t = 496, 50, 3, 0.5
    frames_np = np.stack([oracle_mod.gen_noise(w, h, 700 + i) for i in range(n + 1)])
    frames_np[1, :, :, 3] = 255
    frames = put(frames_np)
    u = _upscaler(nsc, alg, w, h, 2 * w, 2 * h, {"rows_per_wave": 12})
    assert u.kernel_variant == "lanczos3_x2_regwin"
    fb = w * h * 4
    mid = guarded.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
    up_real = guarded.zeros((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device="cuda")
    up_mid = guarded.zeros_like(up_real)
    u.upscale_unit_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, t, mid.data_ptr(), up_real.data_ptr(),
                          up_mid.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got_mid, got_real, got_up_mid = fetch(mid), fetch(up_real), fetch(up_mid)
    for i in range(n):
        m = oracle_mod.warp_blend(frames_np[i], frames_np[i + 1], None, t)
        assert np.array_equal(got_mid[i], m), i
        _record("lanczos3_x2_regwin", alg, check_fma(oracle_mod, got_real[i], frames_np[i], 2 * w, 2 * h, filt, ("unit real", alg, i)))
        _record("lanczos3_x2_regwin", alg, check_fma(oracle_mod, got_up_mid[i], m, 2 * w, 2 * h, filt, ("unit mid", alg, i)))


def test_1080p_to_4k_x2_meets_fma_contract(nsc, oracle_mod):
    """One full frame on the x2 kernel: the opaque gradient (3-channel path) and noise with alpha (4-channel path)."""
    import torch

    w, h = 1920, 1080
    u = _upscaler(nsc, "lanczos3", w, h, 2 * w, 2 * h, {})
    assert u.kernel_variant == "lanczos3_x2_regwin"
    eps = contract_eps(oracle_mod, w, h, 2 * w, 2 * h, 0)
    for name, img in (("gradient", oracle_mod.gen_gradient(w, h, 0)), ("noise", oracle_mod.gen_noise(w, h, 1080))):
        got = _device_batch(torch, u, img[None], 2 * w, 2 * h)[0]
        v = resample64(oracle_mod, img, 2 * w, 2 * h, 0)
        _record("lanczos3_x2_regwin", "lanczos3", assert_fma_contract(got, v, eps, ("1080p -> 4K", name)))
        del got, v


def test_every_resize_variant_was_held_to_the_contract():
    """Runs last: the kernels seen above are exactly the resize variants.  Prints the measured table (pytest -rP shows it)."""
    seen = {v for v, _ in _STATS}
    assert seen == RESIZE_VARIANTS, (sorted(RESIZE_VARIANTS - seen), sorted(seen - RESIZE_VARIANTS))
    for (variant, alg), (samples, differ, worst) in sorted(_STATS.items()):
        print(f"{variant:22s} {alg:9s} samples {samples:10d}  differ from floor(c + 0.5): {differ:7d} "
              f"({differ / samples:.2e})  worst tie distance among them: {worst:.2e}")
