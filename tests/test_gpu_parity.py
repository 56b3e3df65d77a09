"""GPU: parity of the HIP path (through the C ABI) against the CPU oracle.

Bit-exact for nearest and bilinear; Lanczos-3 and warp+blend within +-1 LSB per channel
(the tolerance BASELINE.json's north_star states), with the stricter results the
implementation actually achieves asserted where they hold (EXACT mode: 0 differences).
"""
import os

import numpy as np
import pytest

from _resample64 import check_fma  # the FMA-mode contract: float64 resample, round to nearest, ties either way
from _warp64 import warp_contract  # the FMA-mode warp's contract: float64 samples, truncated, a band at integers
from conftest import GOLDEN, guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch  # host <-> HBM through nus_upload / nus_download, never
# torch's pageable copies (docs/d2h_fault_analysis.md)

pytestmark = pytest.mark.gpu


def _up(nsc, alg, img, ow, oh, **kw):
    opts = kw.pop("options", {})
    u = nsc.PyWgpuUpscaler("quality", alg, **kw)
    for k, v in opts.items():
        u.set_option(k, v)
    ih, iw = img.shape[:2]
    u.initialize(iw, ih, ow, oh)
    out = np.frombuffer(u.upscale(img.tobytes()), dtype=np.uint8).reshape(oh, ow, 4)
    return out, u


def _maxdiff(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


def test_device_present(nsc):
    assert nsc.device_count() >= 1


# ---- sizes: x2 fast paths, general scales, ragged / tiny shapes -------------------

X2_SIZES = [(64, 36), (320, 240), (252, 20), (256, 33), (16, 1), (500, 7), (1000, 50)]
GENERAL = [((64, 36), (96, 54)), ((48, 27), (72, 41)), ((50, 31), (127, 64)), ((37, 21), (74, 42)),
           ((48, 27), (20, 11)), ((1, 1), (5, 3)), ((3, 2), (6, 4)), ((7, 5), (7, 5)), ((97, 13), (101, 29))]


@pytest.mark.parametrize("size", X2_SIZES)
def test_nearest_x2_bit_exact(nsc, oracle_mod, size):
    w, h = size
    img = oracle_mod.gen_noise(w, h, 11)
    out, u = _up(nsc, "nearest", img, 2 * w, 2 * h)
    assert u.kernel_variant == "nearest_x2_vec16"
    assert np.array_equal(out, oracle_mod.nearest(img, 2 * w, 2 * h))
    out_g, ug = _up(nsc, "nearest", img, 2 * w, 2 * h, options={"force_general": 1})
    assert ug.kernel_variant == "nearest_table" and np.array_equal(out_g, out)


@pytest.mark.parametrize("dims", GENERAL)
def test_nearest_general_bit_exact(nsc, oracle_mod, dims):
    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 12)
    out, _ = _up(nsc, "nearest", img, ow, oh)
    assert np.array_equal(out, oracle_mod.nearest(img, ow, oh))


@pytest.mark.parametrize("size", X2_SIZES)
def test_bilinear_x2_bit_exact(nsc, oracle_mod, size):
    w, h = size
    img = oracle_mod.gen_noise(w, h, 13)
    want = oracle_mod.bilinear(img, 2 * w, 2 * h)
    out, u = _up(nsc, "bilinear", img, 2 * w, 2 * h)
    assert u.kernel_variant == "bilinear_x2_packed_u8"
    assert np.array_equal(out, want)
    out_g, ug = _up(nsc, "bilinear", img, 2 * w, 2 * h, options={"force_general": 1})
    assert ug.kernel_variant == "bilinear_table_f32" and np.array_equal(out_g, want)


@pytest.mark.parametrize("dims", GENERAL)
def test_bilinear_general_bit_exact(nsc, oracle_mod, dims):
    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 14)
    out, _ = _up(nsc, "bilinear", img, ow, oh)
    assert np.array_equal(out, oracle_mod.bilinear(img, ow, oh))
    out_w, _ = _up(nsc, "bilinear", img, ow, oh, bilinear_variant="wgsl")
    assert np.array_equal(out_w, oracle_mod.bilinear_wgsl(img, ow, oh))


@pytest.mark.parametrize("ratio", [(3, 2), (4, 3), (3, 1), (4, 1), (2, 1), (5, 4), (6, 5), (5, 3), (5, 2), (7, 2), (7, 5)])
@pytest.mark.parametrize("groups", [(1, 1), (2, 3), (32, 18), (33, 19), (63, 10), (64, 11), (65, 12), (250, 20), (640, 360)])
def test_nearest_and_bilinear_fixed_ratio_kernels(nsc, oracle_mod, ratio, groups):
    """The small rational factors (x3/2 -- the scale the reference's benchmark entry points default to --, x4/3, x3, x4 and, since
    round 5, the P/Q resize kernel's x5/4, x6/5, x5/3, x5/2, x7/2) have their own nearest and CPU-form bilinear kernels (one input group per lane, P outputs; row groups): bit-exact against the
    oracle and the table-driven kernels; the WGSL form keeps the table kernel."""
    P, Q = ratio
    w, h = Q * groups[0], Q * groups[1]
    if (P, Q) in ((4, 1), (7, 2)) and w * h > 100000:
        pytest.skip("covered by the smaller sizes")
    if (P, Q) == (2, 1):
        if w % 4 == 0:
            pytest.skip("x2 at widths % 4 == 0 has its own kernels")
        # (x2 at the other widths -- 1366x768 -- takes the fixed-ratio kernels)
    ow, oh = P * groups[0], P * groups[1]
    img = oracle_mod.gen_noise(w, h, 18)
    want = oracle_mod.bilinear(img, ow, oh)
    out, u = _up(nsc, "bilinear", img, ow, oh)
    # (x5/2, x7/2: the table kernel is the faster one for bilinear, x7/5: the fixed-ratio one does not fit the registers;
    # nearest takes the fixed-ratio kernel at every factor)
    assert u.kernel_variant == ("bilinear_table_f32" if (P, Q) in ((5, 2), (7, 2), (7, 5)) else "bilinear_ratio_f32")
    assert np.array_equal(out, want)
    out_g, ug = _up(nsc, "bilinear", img, ow, oh, options={"force_general": 1})
    assert ug.kernel_variant == "bilinear_table_f32" and np.array_equal(out_g, want)
    out_w, uw = _up(nsc, "bilinear", img, ow, oh, bilinear_variant="wgsl")
    assert uw.kernel_variant == "bilinear_table_f32" and np.array_equal(out_w, oracle_mod.bilinear_wgsl(img, ow, oh))
    ub = nsc.PyWgpuUpscaler("quality", "bilinear")
    ub.set_input_format("bgra")
    ub.initialize(w, h, ow, oh)
    assert np.array_equal(np.frombuffer(ub.upscale(_bgra(img).tobytes()), np.uint8).reshape(oh, ow, 4), want)
    want_n = oracle_mod.nearest(img, ow, oh)
    out_n, un = _up(nsc, "nearest", img, ow, oh)
    assert un.kernel_variant == "nearest_ratio" and np.array_equal(out_n, want_n)
    out_ng, ung = _up(nsc, "nearest", img, ow, oh, options={"force_general": 1})
    assert ung.kernel_variant == "nearest_table" and np.array_equal(out_ng, want_n)


@pytest.mark.parametrize("size", [(64, 36), (320, 240), (252, 20), (256, 33), (16, 1), (500, 7), (1000, 50), (248, 40), (496, 9),
                                  (16, 16), (20, 17), (1916, 23), (128, 97)])
def test_lanczos_x2(nsc, oracle_mod, size):
    w, h = size
    img = oracle_mod.gen_noise(w, h, 15)
    want = oracle_mod.lanczos3(img, 2 * w, 2 * h)
    out, u = _up(nsc, "lanczos3", img, 2 * w, 2 * h)
    # the register-window kernel needs >= 16 rows and columns; smaller frames take the general one
    assert u.kernel_variant == ("lanczos3_x2_regwin" if w >= 16 and h >= 16 else "resize_regwin_lds")
    d = np.abs(out.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1, f"FMA mode outside +-1 LSB (max {d.max()})"
    assert (d > 0).mean() < 1e-3
    # EXACT mode reproduces the oracle's rounding sequence: no differences at all
    out_e, _ = _up(nsc, "lanczos3", img, 2 * w, 2 * h, lanczos_mode="exact")
    assert np.array_equal(out_e, want)
    # the general kernel agrees with the fast one (same weights, same op order)
    out_g, ug = _up(nsc, "lanczos3", img, 2 * w, 2 * h, lanczos_mode="exact", options={"force_general": 1})
    assert ug.kernel_variant == "resize_regwin_lds" and np.array_equal(out_g, want)
    out_r, ur = _up(nsc, "lanczos3", img, 2 * w, 2 * h, lanczos_mode="exact", options={"force_general": 1, "force_rows": 1})
    assert ur.kernel_variant == "resize_rows_lds" and np.array_equal(out_r, want)
    out_p, up_ = _up(nsc, "lanczos3", img, 2 * w, 2 * h, lanczos_mode="exact", options={"force_general": 1, "force_per_pixel": 1})
    assert up_.kernel_variant == "lanczos3_general" and np.array_equal(out_p, want)
    # every rows-per-wave split produces the same image
    for th in (1, 5, 7, 8, 23):
        out_t, _ = _up(nsc, "lanczos3", img, 2 * w, 2 * h, lanczos_mode="exact", options={"rows_per_wave": th})
        assert np.array_equal(out_t, want), th


@pytest.mark.parametrize("dims", GENERAL + [((12, 9), (24, 18)), ((100, 40), (30, 12))])
def test_lanczos_general(nsc, oracle_mod, dims):
    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 16)
    want = oracle_mod.lanczos3(img, ow, oh)
    out, _ = _up(nsc, "lanczos3", img, ow, oh)
    assert _maxdiff(out, want) <= 1
    check_fma(oracle_mod, out, img, ow, oh, 0, ("lanczos3", dims))
    out_e, _ = _up(nsc, "lanczos3", img, ow, oh, lanczos_mode="exact")
    assert np.array_equal(out_e, want)


@pytest.mark.parametrize("alg,filt", [("bicubic", 1), ("triangle", 2)])
@pytest.mark.parametrize("dims", [((64, 36), (128, 72)), ((320, 240), (640, 480)), ((252, 20), (504, 40)), ((48, 27), (72, 41)),
                                  ((50, 31), (127, 64)), ((48, 27), (20, 11)), ((7, 5), (7, 5)), ((12, 9), (24, 18))])
def test_bicubic_and_triangle_resize(nsc, oracle_mod, alg, filt, dims):
    """Next row 8f-4: the other image-0.24.9 filters of the legacy BasicUpscaler (CatmullRom, Triangle),
    through the same table-driven kernels (x2 register-window kernel where it applies)."""
    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 17)
    want = oracle_mod.resize(img, ow, oh, filt)
    out, u = _up(nsc, alg, img, ow, oh)
    x2 = (ow, oh) == (2 * w, 2 * h) and w % 4 == 0 and w >= 16 and h >= 16
    r32 = (2 * ow, 2 * oh) == (3 * w, 3 * h) and w % 8 == 0 and h % 2 == 0 and w >= 32 and h >= 16
    r43 = (3 * ow, 3 * oh) == (4 * w, 4 * h) and w % 12 == 0 and h % 3 == 0 and w >= 48 and h >= 18
    upscale_by4 = ow % 4 == 0 and ow >= w and oh >= h
    assert u.kernel_variant == ("lanczos3_x2_regwin" if x2 else "lanczos3_r32_regwin" if r32 else "lanczos3_r43_regwin" if r43 else
                                ("resize_regwin_lds" if upscale_by4 else ("resize_down_stream" if oh < h else "resize_rows_lds")))
    assert _maxdiff(out, want) <= 1
    check_fma(oracle_mod, out, img, ow, oh, filt, (alg, dims, u.kernel_variant))
    out_e, _ = _up(nsc, alg, img, ow, oh, lanczos_mode="exact")
    assert np.array_equal(out_e, want)
    assert u.name == {"bicubic": "HipBicubicUpscaler", "triangle": "HipTriangleUpscaler"}[alg]


def test_table_blob_filter_mismatch_rejected(nsc):
    u = nsc.PyWgpuUpscaler("quality", "bicubic")
    u.initialize(64, 36, 128, 72)
    assert u.export_tables() == nsc.build_tables_blob(64, 36, 128, 72, algorithm="bicubic")
    with pytest.raises(RuntimeError, match="different resize filter"):
        u.import_tables(nsc.build_tables_blob(64, 36, 128, 72, algorithm="lanczos3"))


def test_lanczos_unsupported_ratio_errors(nsc, oracle_mod):
    u = nsc.PyWgpuUpscaler("quality", "lanczos3")
    with pytest.raises(RuntimeError, match="exceeds 32 taps"):
        u.initialize(1000, 8, 100, 8)


# ---- the reference's own fixtures, through the GPU ----------------------------------

def test_reference_bilinear_fixture(nsc, golden):
    for variant in ("cpu", "wgsl"):
        out, _ = _up(nsc, "bilinear", golden["test_input"], 640, 480, bilinear_variant=variant)
        assert np.array_equal(out[:240, :320], golden["test_output"][:240, :320])


def test_reference_interp_fixture(nsc, oracle_mod, golden):
    a = oracle_mod.gen_box(64, 64, (255, 0, 0, 255))
    b = oracle_mod.gen_box(64, 64, (0, 0, 255, 255))
    it = nsc.WgpuFrameInterpolator()
    assert it.get_last_gpu_duration_ms() is None
    out = np.frombuffer(it.interpolate_py(a.tobytes(), b.tobytes(), 64, 64, time_t=0.5), np.uint8).reshape(64, 64, 4)
    assert np.array_equal(out, golden["interp_half"])
    assert it.get_last_gpu_duration_ms() is not None
    # the same through the shape of trait FrameInterpolator (interpolation/mod.rs:29-44): initialize, then interpolate(f1, f2, t)
    tr = nsc.WgpuFrameInterpolator()
    tr.initialize(64, 64)
    tr.initialize(64, 64)  # same size again: no-op
    out = np.frombuffer(tr.interpolate(a.tobytes(), b.tobytes(), 0.5), np.uint8).reshape(64, 64, 4)
    assert np.array_equal(out, golden["interp_half"])
    with pytest.raises(ValueError, match="Expected 16384 bytes per frame for 64x64x4 RGBA"):
        tr.interpolate(a.tobytes()[:-4], b.tobytes()[:-4], 0.5)


def test_committed_oracle_vectors(nsc):
    import oracle as oracle_mod

    v = np.load(os.path.join(GOLDEN, "oracle_vectors.npz"))
    noise = v["noise_48x27"]
    for name, (ow, oh) in {"x2": (96, 54), "x1p5": (72, 41), "down": (20, 11)}.items():
        assert np.array_equal(_up(nsc, "nearest", noise, ow, oh)[0], v[f"nearest_{name}"])
        assert np.array_equal(_up(nsc, "bilinear", noise, ow, oh)[0], v[f"bilinear_{name}"])
        assert np.array_equal(_up(nsc, "bilinear", noise, ow, oh, bilinear_variant="wgsl")[0], v[f"bilinear_wgsl_{name}"])
        got_f = _up(nsc, "lanczos3", noise, ow, oh)[0]
        assert _maxdiff(got_f, v[f"lanczos3_{name}"]) <= 1
        check_fma(oracle_mod, got_f, noise, ow, oh, 0, ("lanczos3", name))
    it = nsc.WgpuFrameInterpolator()
    a, b, flow = v["warp_a"], v["warp_b"], v["warp_flow"]
    h, w = a.shape[:2]
    for key, fl, t in (("warp_zero_t050", None, 0.5), ("warp_zero_t030", None, 0.3), ("warp_flow_t050", flow, 0.5),
                       ("warp_flow_t025", flow, 0.25)):
        out = np.frombuffer(it.interpolate_py(a.tobytes(), b.tobytes(), w, h, time_t=t, flow=fl), np.uint8).reshape(h, w, 4)
        assert np.array_equal(out, v[key]), key
    # next rows: EXACT mode reproduces the committed bytes, FMA mode stays within 1 LSB
    small = v["noise_24x14"]
    for alg, src, (ow, oh), key in (("bicubic", small, (48, 28), "catmullrom_x2"), ("triangle", small, (36, 21), "triangle_x1p5"),
                                    ("lanczos3", small, (96, 56), "lanczos3_x4"), ("lanczos3", noise, (24, 13), "lanczos3_half"),
                                    ("bicubic", noise, (16, 9), "catmullrom_third"),
                                    # round 5: the P/Q register-window kernel's factors
                                    ("lanczos3", v["noise_40x15"], (48, 18), "lanczos3_x6o5"), ("bicubic", v["noise_40x15"], (56, 21), "catmullrom_x7o5"),
                                    ("lanczos3", v["noise_36x12"], (60, 20), "lanczos3_x5o3"), ("triangle", v["noise_36x12"], (60, 20), "triangle_x5o3"),
                                    ("lanczos3", v["noise_32x12"], (40, 15), "lanczos3_x5o4"), ("lanczos3", v["noise_32x12"], (80, 30), "lanczos3_x5o2")):
        got_e, ue = _up(nsc, alg, src, ow, oh, lanczos_mode="exact")
        assert np.array_equal(got_e, v[key]), key
        got_f = _up(nsc, alg, src, ow, oh)[0]
        assert _maxdiff(got_f, v[key]) <= 1, key
        check_fma(oracle_mod, got_f, src, ow, oh, {"lanczos3": 0, "bicubic": 1, "triangle": 2}[alg], key)
        if key in ("lanczos3_x6o5", "catmullrom_x7o5", "lanczos3_x5o3", "triangle_x5o3", "lanczos3_x5o4", "lanczos3_x5o2"):
            assert ue.kernel_variant == "lanczos3_pq_regwin", (key, ue.kernel_variant)
    u = nsc.PyWgpuUpscaler("quality", "fsr1")
    u.set_sharpness(0.0, 0.7)
    u.initialize(24, 14, 48, 28)
    assert np.array_equal(np.frombuffer(u.upscale(small.tobytes()), np.uint8).reshape(28, 48, 4), v["fsr1_x2"])
    fe = nsc.FlowEstimator(levels=2, coarse_iterations=5, refine_iterations=2)
    assert np.array_equal(fe.estimate(a, b, w, h), v["flow_l2_c5_r2"])


# ---- warp + blend ---------------------------------------------------------------------

@pytest.mark.parametrize("size", [(64, 48), (61, 7), (1, 1), (256, 4), (130, 33)])
@pytest.mark.parametrize("t", [0.5, 0.0, 1.0, 0.3])
def test_warp_blend_vs_oracle(nsc, oracle_mod, size, t):
    w, h = size
    a = oracle_mod.gen_noise(w, h, 21)
    b = oracle_mod.gen_noise(w, h, 22)
    rng = np.random.default_rng(w * 1000 + h)
    flow = (rng.standard_normal((h, w, 2)) * 5).astype(np.float32)
    flow[0, 0] = (1000.0, -1000.0)  # far outside: exercises the clamp
    it = nsc.WgpuFrameInterpolator("16x16")
    for fl in (None, flow):
        out = np.frombuffer(it.interpolate_py(a.tobytes(), b.tobytes(), w, h, time_t=t, flow=fl), np.uint8).reshape(h, w, 4)
        want = oracle_mod.warp_blend(a, b, fl, t)
        assert np.array_equal(out, want), (size, t, fl is not None, _maxdiff(out, want))
    if t == 0.0:
        assert np.array_equal(out if fl is None else np.frombuffer(it.interpolate_py(a.tobytes(), b.tobytes(), w, h, time_t=0.0), np.uint8).reshape(h, w, 4), a)


def test_warp_constant_flow_recovers_shifted_stream(nsc, oracle_mod):
    """Stream frames k and k+1 differ by a 1 px shift; with the true constant flow the
    in-between frame at t=0.5 is the half-pixel shift of frame k (away from the wrap column)."""
    w, h = 128, 16
    a = oracle_mod.gen_gradient(w, h, 10)
    b = oracle_mod.gen_gradient(w, h, 11)
    # content moves left by one pixel per frame: A(x) = B(x-1)  =>  flow = (-1, 0)
    flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0] = -1.0
    it = nsc.WgpuFrameInterpolator()
    out = np.frombuffer(it.interpolate_py(a.tobytes(), b.tobytes(), w, h, time_t=0.5, flow=flow), np.uint8).reshape(h, w, 4)
    assert np.array_equal(out, oracle_mod.warp_blend(a, b, flow, 0.5))


@pytest.mark.parametrize("size", [(64, 48), (61, 7), (2, 2), (256, 4), (130, 33), (1, 5), (7, 1), (1920, 1080)])
def test_warp_blend_fma_mode_within_one_lsb(nsc, oracle_mod, size):
    """NUS_INTERP_MODE_FMA of the dense-flow warp (fused lerps): every sample within 1 LSB of the oracle and fewer than
    0.1 % of them different -- noise frames, sub-pixel flows everywhere, far-outside vectors, frame borders, widths that
    take the 4-pixels-per-lane kernel and widths that do not, frames too small for the corner sampler, f32 and f16 flow
    fields.  EXACT mode on the same inputs: bit-exact."""
    import torch

    w, h = size
    n = 2 if w * h > 100000 else 3
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(w * 7 + h)
    frames_np = np.stack([oracle_mod.gen_noise(w, h, 900 + i) for i in range(n + 1)])
    flow = (rng.standard_normal((n, h, w, 2)) * 6).astype(np.float32)
    flow[:, 0, 0] = (1000.0, -1000.0)
    flow[:, -1, -1] = (-0.25, 7.5)
    frames = put(frames_np)
    fb = w * h * 4
    s = torch.cuda.current_stream().cuda_stream
    it = nsc.WgpuFrameInterpolator()
    assert it.mode == "exact"
    out = guarded.zeros((n, h, w, 4), dtype=torch.uint8, device=dev)
    for t in (0.5, 0.3):
        for fmt in ("f32", "f16"):
            fl_np = flow if fmt == "f32" else flow.astype(np.float16)
            d_flow = put(fl_np)
            it.set_flow_format(fmt)
            want = [oracle_mod.warp_blend(frames_np[i], frames_np[i + 1], fl_np[i].astype(np.float32), t, threads=0) for i in range(n)]
            for mode in ("exact", "fma"):
                it.set_mode(mode)
                out.zero_()
                it.interpolate_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, d_flow.data_ptr(), w, h, t, out.data_ptr(), n, s)
                torch.cuda.synchronize()
                got = fetch(out)
                for i in range(n):
                    if mode == "exact":
                        assert np.array_equal(got[i], want[i]), (size, t, fmt, i)
                    else:
                        d = np.abs(got[i].astype(np.int16) - want[i].astype(np.int16))
                        assert d.max() <= 1, (size, t, fmt, i, int(d.max()))
                        assert (d > 0).mean() < 1e-3 or d.size < 4000, (size, t, fmt, i, float((d > 0).mean()))
                        if w * h < 1920 * 1080:  # the float64 contract (tests/_warp64.py); frames below 2 x 2 run EXACT arithmetic
                            warp_contract(got[i], frames_np[i], frames_np[i + 1], fl_np[i], t, 0.5 if min(w, h) >= 2 else 1.0,
                                          (size, t, fmt, i))
    # host entry point in FMA mode; zero flow stays the exact blend
    it.set_mode("fma")
    it.set_flow_format("f32")
    a, b = frames_np[0], frames_np[1]
    got = np.frombuffer(it.interpolate_py(a.tobytes(), b.tobytes(), w, h, time_t=0.5, flow=flow[0]), np.uint8).reshape(h, w, 4)
    assert np.abs(got.astype(np.int16) - oracle_mod.warp_blend(a, b, flow[0], 0.5).astype(np.int16)).max() <= 1
    z = np.frombuffer(it.interpolate_py(a.tobytes(), b.tobytes(), w, h, time_t=0.5), np.uint8).reshape(h, w, 4)
    assert np.array_equal(z, oracle_mod.warp_blend(a, b, None, 0.5))
    with pytest.raises(ValueError):
        it.set_mode("fast")


def test_warp_blend_with_f16_flow_field(nsc, oracle_mod):
    """NUS_FLOW_F16: the Rg16Float flow layout of the reference's live path (wgpu_interpolator.rs:276).  Each half widens
    to f32 exactly, so the result equals the oracle run on the f16-rounded flow bit for bit; against the unrounded f32
    flow it stays within one count almost everywhere (a quarter-pixel flow has ~1e-3 px of f16 rounding)."""
    import torch

    w, h, n = 130, 33, 3
    rng = np.random.default_rng(12)
    frames_np = np.stack([oracle_mod.gen_noise(w, h, 300 + i) for i in range(n + 1)])
    flow32 = (rng.random((n, h, w, 2)) * 8.0 - 4.0).astype(np.float32)
    flow16 = flow32.astype(np.float16)
    dev = torch.device("cuda:0")
    frames = put(frames_np)
    d_flow16 = put(flow16)
    out = guarded.zeros((n, h, w, 4), dtype=torch.uint8, device=dev)
    it = nsc.WgpuFrameInterpolator()
    it.set_flow_format("f16")
    fb = w * h * 4
    it.interpolate_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, d_flow16.data_ptr(), w, h, 0.5, out.data_ptr(), n,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = fetch(out)
    for i in range(n):
        want = oracle_mod.warp_blend(frames_np[i], frames_np[i + 1], flow16[i].astype(np.float32), 0.5)
        assert np.array_equal(got[i], want), i
        full = oracle_mod.warp_blend(frames_np[i], frames_np[i + 1], flow32[i], 0.5)
        # noise frames: a sample position moved by the flow's f16 rounding (up to 2e-3 px) changes a truncated sample by a
        # count now and then; never by more than a few
        d = np.abs(got[i].astype(np.int16) - full.astype(np.int16))
        assert d.max() <= 2 and (d > 0).mean() < 0.15, (i, int(d.max()), float((d > 0).mean()))
    # back to f32: the same entry point reads 8 bytes per pixel again
    it.set_flow_format("f32")
    d_flow32 = put(flow32)
    it.interpolate_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, d_flow32.data_ptr(), w, h, 0.5, out.data_ptr(), n,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(fetch(out[0]), oracle_mod.warp_blend(frames_np[0], frames_np[1], flow32[0], 0.5))
    with pytest.raises(ValueError):
        it.set_flow_format("bf16")


def test_interp_size_mismatch_raises_valueerror(nsc):
    it = nsc.WgpuFrameInterpolator()
    with pytest.raises(ValueError, match="Expected 64 bytes per frame for 4x4x4 RGBA"):
        it.interpolate_py(b"\0" * 64, b"\0" * 63, 4, 4)


# ---- host API behaviour on the GPU -----------------------------------------------------

def test_upscale_errors_and_reinit(nsc, oracle_mod):
    u = nsc.PyWgpuUpscaler("quality", "bilinear")
    u.initialize(8, 8, 16, 16)
    with pytest.raises(RuntimeError, match=r"Input data size \(12\) does not match expected input buffer size \(256 for 8x8\)"):
        u.upscale(b"\0" * 12)
    img = oracle_mod.gen_noise(8, 8, 5)
    assert np.array_equal(np.frombuffer(u.upscale(img.tobytes()), np.uint8).reshape(16, 16, 4), oracle_mod.bilinear(img, 16, 16))
    u.initialize(10, 6, 25, 9)  # re-init with new dimensions (upscale/mod.rs:883-889)
    assert abs(u.upscale_scale - (2.5 + 1.5) / 2) < 1e-6
    img = oracle_mod.gen_noise(10, 6, 6)
    assert np.array_equal(np.frombuffer(u.upscale(img.tobytes()), np.uint8).reshape(9, 25, 4), oracle_mod.bilinear(img, 25, 9))
    assert u.get_last_gpu_duration_ms() is not None


@pytest.mark.parametrize("alg", ["nearest", "bilinear", "lanczos3"])
def test_upscale_batch_matches_single(nsc, oracle_mod, alg):
    w, h = 96, 40
    frames = [oracle_mod.gen_noise(w, h, 100 + i) for i in range(7)]  # > 2x the 3 pipeline slots
    u = nsc.PyWgpuUpscaler("quality", alg, lanczos_mode="exact")
    u.initialize(w, h, 2 * w, 2 * h)
    outs = u.upscale_batch([f.tobytes() for f in frames])
    ref = {"nearest": oracle_mod.nearest, "bilinear": oracle_mod.bilinear, "lanczos3": oracle_mod.lanczos3}[alg]
    assert len(outs) == 7
    for f, o in zip(frames, outs):
        assert np.array_equal(np.frombuffer(o, np.uint8).reshape(2 * h, 2 * w, 4), ref(f, 2 * w, 2 * h))
    assert u.upscale_batch([]) == []


def test_upscale_batch_pipeline_many_frames_every_buffer_kind(nsc, oracle_mod):
    """The pipelined batch (submitting thread + retiring thread + copy pool): more frames than slots at a size whose
    output comes back in several pieces, into fresh bytes, into caller-owned pageable buffers and into pinned ones,
    repeatedly on one handle; a bad frame in the middle of a batch fails the call and leaves the handle usable."""
    import torch

    w, h, n = 640, 360, 11  # 3.7 MB out per frame: 8 pieces of ~460 KB, each copy split over the pool
    frames = [oracle_mod.gen_noise(w, h, 4000 + i) for i in range(n)]
    want = [oracle_mod.bilinear(f, 2 * w, 2 * h) for f in frames]
    u = nsc.PyWgpuUpscaler("quality", "bilinear")
    u.initialize(w, h, 2 * w, 2 * h)
    ins = [f.tobytes() for f in frames]
    for _ in range(2):
        outs = u.upscale_batch(ins)
        assert all(np.array_equal(np.frombuffer(o, np.uint8).reshape(2 * h, 2 * w, 4), wnt) for o, wnt in zip(outs, want))
    bufs = [bytearray(u.output_size) for _ in range(n)]
    u.upscale_batch_into(ins, bufs)
    assert all(np.array_equal(np.frombuffer(b, np.uint8).reshape(2 * h, 2 * w, 4), wnt) for b, wnt in zip(bufs, want))
    pin_in = torch.empty((n, u.input_size), dtype=torch.uint8, pin_memory=True)
    pin_out = torch.zeros((n, u.output_size), dtype=torch.uint8, pin_memory=True)
    for k in range(n):
        pin_in[k] = torch.from_numpy(frames[k].reshape(-1))
    u.upscale_batch_into([pin_in[k].numpy() for k in range(n)], [pin_out[k].numpy() for k in range(n)])
    assert all(np.array_equal(pin_out[k].numpy().reshape(2 * h, 2 * w, 4), want[k]) for k in range(n))
    # mixed: pinned inputs, pageable outputs, and a single-frame batch
    u.upscale_batch_into([pin_in[k].numpy() for k in range(n)], bufs)
    assert np.array_equal(np.frombuffer(bufs[n - 1], np.uint8).reshape(2 * h, 2 * w, 4), want[n - 1])
    one = [bytearray(u.output_size)]
    u.upscale_batch_into(ins[4:5], one)
    assert np.array_equal(np.frombuffer(one[0], np.uint8).reshape(2 * h, 2 * w, 4), want[4])
    # caller-owned buffers pinned in place (nus_host_pin): the DMA engines write straight into the bytearrays
    pinned = [nsc.PinnedBuffer(b) for b in bufs]
    for b in bufs:
        b[:] = bytes(len(b))
    u.upscale_batch_into(ins, bufs)
    assert all(np.array_equal(np.frombuffer(b, np.uint8).reshape(2 * h, 2 * w, 4), wnt) for b, wnt in zip(bufs, want))
    with pinned[0] as b0:  # context-manager form: unpinned on exit, the buffer stays usable
        u.upscale_into(ins[3], b0)
        assert np.array_equal(np.frombuffer(b0, np.uint8).reshape(2 * h, 2 * w, 4), want[3])
    for pb in pinned:
        pb.unpin()
    u.upscale_batch_into(ins, bufs)  # pageable again
    assert np.array_equal(np.frombuffer(bufs[1], np.uint8).reshape(2 * h, 2 * w, 4), want[1])
    with pytest.raises(TypeError):
        nsc.PinnedBuffer(b"read-only")
    bad = list(ins)
    bad[6] = bad[6][:-4]
    with pytest.raises(RuntimeError, match="does not match expected input buffer size"):
        u.upscale_batch(bad)
    assert np.array_equal(np.frombuffer(u.upscale(ins[2]), np.uint8).reshape(2 * h, 2 * w, 4), want[2])


def test_failed_retire_mid_batch_leaves_nothing_queued(nsc, oracle_mod, monkeypatch):
    """A frame whose wait fails in the middle of a batch (test hook "inject_retire_error": what a lost device looks like) fails the
    call -- and every frame that had been SUBMITTED is still retired: before round 5 the retiring thread left at the first failure,
    the populate requests of the frames in the other slots stayed queued in the process-wide pool with pointers into the result
    buffers the caller frees next and into the slots' tickets inside the upscaler.  Checked at 1080p -> 4K with fresh
    `bytes` results (33 MB each: the buffers that get populate requests), for the batch, the single call and the ring: nothing
    is pending when the failing call returns, the handle can be destroyed at once, and a new one computes correct frames."""
    import gc

    u = nsc.PyWgpuUpscaler("quality", "bilinear")
    monkeypatch.delenv("NUS_TEST_HOOKS", raising=False)
    with pytest.raises(RuntimeError, match="unknown option 'inject_retire_error'"):
        u.set_option("inject_retire_error", 1)  # the production library does not know the hook unless the process asks for hooks
    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    w, h, n = 1920, 1080, 7
    frames = [oracle_mod.gen_noise(w, h, 900 + i) for i in range(2)]
    want = [oracle_mod.bilinear(f, 2 * w, 2 * h, threads=0) for f in frames]
    ins = [frames[i % 2].tobytes() for i in range(n)]
    lib = nsc._capi.lib()
    for fail_at in (1, 2, 3, 5):
        u = nsc.PyWgpuUpscaler("quality", "bilinear")
        u.initialize(w, h, 2 * w, 2 * h)
        u.set_option("inject_retire_error", fail_at)
        with pytest.raises(RuntimeError, match="HIP error in hipEventSynchronize"):
            u.upscale_batch(ins)
        assert lib.nus_host_pending_pieces() == 0, fail_at
        del u
        gc.collect()
        assert lib.nus_host_pending_pieces() == 0
    u = nsc.PyWgpuUpscaler("quality", "bilinear")
    u.initialize(w, h, 2 * w, 2 * h)
    u.set_option("inject_retire_error", 1)
    with pytest.raises(RuntimeError, match="HIP error in hipEventSynchronize"):
        u.upscale(ins[0])
    assert lib.nus_host_pending_pieces() == 0
    outs = u.upscale_batch(ins)  # the same handle goes on working
    assert all(np.array_equal(np.frombuffer(o, np.uint8).reshape(2 * h, 2 * w, 4), want[i % 2]) for i, o in enumerate(outs))
    # the ring: the failure is sticky, every submitted frame is still retired before stream_close returns
    bufs = [bytearray(u.output_size) for _ in range(4)]
    u.stream_open()
    u.set_option("inject_retire_error", 2)
    tickets = []
    try:
        for i in range(4):
            tickets.append(u.stream_submit(ins[i], bufs[i]))
    except RuntimeError:
        pass
    with pytest.raises(RuntimeError):
        u.stream_close()
    assert lib.nus_host_pending_pieces() == 0
    del bufs, u
    gc.collect()
    u = nsc.PyWgpuUpscaler("quality", "bilinear")
    u.initialize(w, h, 2 * w, 2 * h)
    assert np.array_equal(np.frombuffer(u.upscale(ins[1]), np.uint8).reshape(2 * h, 2 * w, 4), want[1])


def test_probe_one_read_four_writes_refuses_partial_waves(nsc):
    """nus_probe_device kind 4 writes four contiguous KiB per wave: a size that is not a whole number of waves (1 KiB of input each)
    used to store up to 3 KiB past 4 * bytes; now it is refused, and whole waves write exactly 4 * bytes."""
    import torch

    dev = torch.device("cuda:0")
    lib = nsc._capi.lib()
    src = torch.arange(0, 4096, dtype=torch.int32, device=dev)  # 16 KiB
    dst = torch.full((4 * 4096 + 4096,), -1, dtype=torch.int32, device=dev)  # 4 x 16 KiB + a guard
    for bad in (16, 1008, 1040, 16 * 1024 - 16):
        assert lib.nus_probe_device(4, src.data_ptr(), dst.data_ptr(), bad, 0, None) == nsc._capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert int((dst != -1).sum()) == 0
    assert lib.nus_probe_device(4, src.data_ptr(), dst.data_ptr(), 16 * 1024, 0, None) == nsc._capi.OK
    torch.cuda.synchronize()
    assert int((dst[:4 * 4096] == -1).sum()) == 0 and int((dst[4 * 4096:] != -1).sum()) == 0


def test_stream_ring_frames_in_one_at_a_time(nsc, oracle_mod):
    """The persistent ring (nus_upscaler_stream_*): 20 frames submitted one by one with three in flight, results in order into
    caller-owned buffers (pageable and pinned), waited for from another thread; the other host entry points are refused while
    the stream is open; closing with frames in flight completes them; re-opening works."""
    import threading

    w, h, n = 320, 180, 20
    frames = [oracle_mod.gen_noise(w, h, 7000 + i) for i in range(n)]
    want = [oracle_mod.bilinear(f, 2 * w, 2 * h) for f in frames]
    u = nsc.PyWgpuUpscaler("quality", "bilinear")
    u.initialize(w, h, 2 * w, 2 * h)
    outs = [bytearray(u.output_size) for _ in range(n)]
    pin = nsc.PinnedBuffer(outs[5])
    u.stream_open()
    with pytest.raises(RuntimeError, match="already open"):
        u.stream_open()
    with pytest.raises(RuntimeError, match="a stream is open"):
        u.upscale(frames[0].tobytes())
    done = []

    def waiter(tickets):
        for t in tickets:
            u.stream_wait(t)
            done.append(t)

    tickets = [u.stream_submit(frames[i].tobytes(), outs[i]) for i in range(8)]
    assert tickets == list(range(8))
    th = threading.Thread(target=waiter, args=(tickets,))
    th.start()
    tickets2 = [u.stream_submit(frames[i].tobytes(), outs[i]) for i in range(8, n)]  # submits while the other thread waits
    th.join()
    assert done == list(range(8))
    with pytest.raises(RuntimeError, match="does not match expected input buffer size"):
        u.stream_submit(frames[0].tobytes()[:-4], outs[0])
    u.stream_wait(tickets2[-3])
    with pytest.raises(RuntimeError, match="no such frame"):
        u.stream_wait(n + 5)
    u.stream_close()  # the last two frames were still in flight
    pin.unpin()
    for i in range(n):
        assert np.array_equal(np.frombuffer(outs[i], np.uint8).reshape(2 * h, 2 * w, 4), want[i]), i
    assert np.array_equal(np.frombuffer(u.upscale(frames[3].tobytes()), np.uint8).reshape(2 * h, 2 * w, 4), want[3])
    u.stream_open()
    out = bytearray(u.output_size)
    u.stream_wait(u.stream_submit(frames[9].tobytes(), out))
    assert np.array_equal(np.frombuffer(out, np.uint8).reshape(2 * h, 2 * w, 4), want[9])
    u.initialize(w, h, 2 * w, 2 * h)  # re-initialising closes the stream
    with pytest.raises(RuntimeError, match="no stream is open"):
        u.stream_submit(frames[0].tobytes(), out)


def test_table_export_import_roundtrip(nsc, oracle_mod):
    img = oracle_mod.gen_noise(64, 36, 3)
    u1 = nsc.PyWgpuUpscaler("quality", "lanczos3", lanczos_mode="exact")
    u1.initialize(64, 36, 128, 72)
    blob = u1.export_tables()
    assert blob == nsc.build_tables_blob(64, 36, 128, 72)
    u2 = nsc.PyWgpuUpscaler("quality", "lanczos3", lanczos_mode="exact")
    u2.initialize(64, 36, 128, 72)
    u2.import_tables(blob)
    assert u2.kernel_variant == "lanczos3_x2_regwin"
    assert u1.upscale(img.tobytes()) == u2.upscale(img.tobytes())
    with pytest.raises(RuntimeError, match="different dimensions"):
        u2.import_tables(nsc.build_tables_blob(64, 36, 96, 54))


_PLAN_CASES = [  # one smallest-size case per variant family: (algorithm, (iw, ih), (ow, oh), the option of the fixture's option set)
    ("lanczos3", (16, 16), (32, 32), None), ("lanczos3", (16, 16), (48, 48), None), ("lanczos3", (16, 16), (64, 64), None),
    ("lanczos3", (32, 16), (48, 24), None), ("lanczos3", (48, 18), (64, 24), None), ("lanczos3", (32, 12), (40, 15), None),
    ("bicubic", (32, 12), (40, 15), None),  # the same factor with a support-2 filter: pq_narrow_active
    ("lanczos3", (100, 60), (237, 141), "force_general"), ("lanczos3", (100, 60), (237, 141), "force_rows"),
    ("lanczos3", (32, 12), (48, 18), None),  # the register-window any-scale kernel, two outputs per lane
    ("lanczos3", (64, 64), (32, 32), None), ("lanczos3", (100, 60), (237, 141), "force_per_pixel"),
    ("nearest", (32, 12), (48, 18), None), ("bilinear", (32, 12), (48, 18), None)]


@pytest.fixture(scope="module")
def kernel_plan_fixture():
    import json
    with open(os.path.join(GOLDEN, "kernel_plan_parent.json")) as f:
        doc = json.load(f)
    return {c["id"]: dict(zip(doc["scalars"], c["s"]), variant=c["variant"]) for c in doc["cases"]}


@pytest.mark.parametrize("alg,size,out,option", _PLAN_CASES)
def test_handle_runs_the_recorded_kernel_plan(nsc, oracle_mod, kernel_plan_fixture, alg, size, out, option):
    """The handle runs what plan_kernels() decides: after initialize() the kernel variant and the plan fields get_option reports are
    those of tests/golden/kernel_plan_parent.json (the CPU test holds every field of every case to that file), and after
    import_tables(export_tables()) -- the second selection on a live handle -- they are the same again and one seeded frame
    comes out byte for byte as before."""
    (w, h), (ow, oh) = size, out
    want = kernel_plan_fixture[f"{alg} {w}x{h}->{ow}x{oh} {option or 'defaults'}"]
    pq, win = want["variant"] == "lanczos3_pq_regwin", want["variant"] == "resize_regwin_lds"
    want_options = {"pq_p": want["pq_p"] if pq else 0, "pq_q": want["pq_q"] if pq else 0,
                    "pq_narrow_active": want["pq_narrow"] if pq else 0,
                    "win_outputs_per_lane": want["win_outputs_per_lane"] if win else 0}
    img = oracle_mod.gen_noise(w, h, 31)
    before, u = _up(nsc, alg, img, ow, oh, options={option: 1} if option else {})
    assert u.kernel_variant == want["variant"]
    assert {k: u.get_option(k) for k in want_options} == want_options
    u.import_tables(u.export_tables())
    assert u.kernel_variant == want["variant"]
    assert {k: u.get_option(k) for k in want_options} == want_options
    assert u.upscale(img.tobytes()) == before.tobytes()


# ---- device-resident batched path (what the bench times) -------------------------------

def test_device_batch_path_matches_host_path(nsc, oracle_mod):
    import torch

    w, h, n = 128, 24, 5
    dev = torch.device("cuda:0")
    frames_np = np.stack([oracle_mod.gen_noise(w, h, 200 + i) for i in range(n + 1)])
    frames = put(frames_np)
    for alg, ref in (("nearest", oracle_mod.nearest), ("bilinear", oracle_mod.bilinear), ("lanczos3", oracle_mod.lanczos3)):
        u = nsc.PyWgpuUpscaler("quality", alg, lanczos_mode="exact")
        u.initialize(w, h, 2 * w, 2 * h)
        out = guarded.zeros((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device=dev)
        u.upscale_device(frames.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = fetch(out)
        for i in range(n):
            assert np.array_equal(got[i], ref(frames_np[i], 2 * w, 2 * h)), (alg, i)
    pipe = nsc.FramePipeline(w, h, 2, "lanczos3", 0.5, lanczos_mode="exact")
    mid, up_real, up_mid = guarded.like(pipe.alloc(n, dev))
    pipe.step(frames, mid, up_real, up_mid, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for i in range(n):
        m = oracle_mod.warp_blend(frames_np[i], frames_np[i + 1], None, 0.5)
        assert np.array_equal(fetch(mid[i]), m)
        assert np.array_equal(fetch(up_real[i]), oracle_mod.lanczos3(frames_np[i], 2 * w, 2 * h))
        assert np.array_equal(fetch(up_mid[i]), oracle_mod.lanczos3(m, 2 * w, 2 * h))


# ---- BASELINE.json configurations at full size -----------------------------------------

def test_config1_1080p_to_4k_bilinear_bit_exact(nsc, oracle_mod):
    for img in (oracle_mod.gen_gradient(1920, 1080, 0), oracle_mod.gen_noise(1920, 1080)):
        out, u = _up(nsc, "bilinear", img, 3840, 2160)
        assert u.kernel_variant == "bilinear_x2_packed_u8"
        assert np.array_equal(out, oracle_mod.bilinear(img, 3840, 2160, threads=0))
        # size-independent property: even output samples are the input itself
        assert np.array_equal(out[::2, ::2], img)


def test_config0_nearest_fixture_and_full_size(nsc, oracle_mod, golden):
    out, _ = _up(nsc, "nearest", golden["test_input"], 640, 480)
    assert np.array_equal(out, np.repeat(np.repeat(golden["test_input"], 2, 0), 2, 1))
    img = oracle_mod.gen_noise(1920, 1080)
    out, _ = _up(nsc, "nearest", img, 3840, 2160)
    assert np.array_equal(out, np.repeat(np.repeat(img, 2, 0), 2, 1))
    img256 = oracle_mod.gen_gradient(256, 256, 0)  # the 256x256 case BASELINE.json words
    out, _ = _up(nsc, "nearest", img256, 512, 512)
    assert np.array_equal(out, oracle_mod.nearest(img256, 512, 512))


def test_config2_1080p_to_4k_lanczos(nsc, oracle_mod):
    img = oracle_mod.gen_noise(1920, 1080)
    want = oracle_mod.lanczos3(img, 3840, 2160, threads=0)
    out, u = _up(nsc, "lanczos3", img, 3840, 2160)
    assert u.kernel_variant == "lanczos3_x2_regwin"
    d = np.abs(out.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    out_e, _ = _up(nsc, "lanczos3", img, 3840, 2160, lanczos_mode="exact")
    assert np.array_equal(out_e, want)
    # size-independent properties: a constant image stays constant; range preserved
    flat = np.full((1080, 1920, 4), 173, np.uint8)
    out_f, _ = _up(nsc, "lanczos3", flat, 3840, 2160)
    assert (out_f == 173).all()


def test_bench_launch_shape_1080p_batch_rows_per_wave_36(nsc, oracle_mod):
    """The exact launch shape bench.py times: a device-resident batch at 1080p -> 4K with 36 input rows per
    wave (what a 300-frame batch auto-selects, nus_host.cpp), on the opaque gradient stream (3-channel path)
    and on noise (4-channel path), through upscale_device and through the fused upscale_blend_device."""
    import torch

    w, h, n = 1920, 1080, 8
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for pattern in ("gradient", "noise"):
        gen = (lambda k: oracle_mod.gen_gradient(w, h, k)) if pattern == "gradient" else (lambda k: oracle_mod.gen_noise(w, h, 900 + k))
        frames_np = np.stack([gen(k) for k in range(n + 1)])
        frames = put(frames_np)
        u = nsc.PyWgpuUpscaler("quality", "lanczos3")
        u.set_option("rows_per_wave", 36)
        u.initialize(w, h, 2 * w, 2 * h)
        assert u.kernel_variant == "lanczos3_x2_regwin"
        out = guarded.zeros((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device=dev)
        u.upscale_device(frames.data_ptr(), out.data_ptr(), n, st)
        fused = guarded.zeros((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device=dev)
        fb = w * h * 4
        u.upscale_blend_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, 0.5, fused.data_ptr(), n, st)
        torch.cuda.synchronize()
        for k in (0, 3, n - 1):
            want = oracle_mod.lanczos3(frames_np[k], 2 * w, 2 * h, threads=0).astype(np.int16)
            d = np.abs(fetch(out[k]).astype(np.int16) - want)
            assert d.max() <= 1 and (d > 0).mean() < 1e-3, (pattern, k, int(d.max()), float((d > 0).mean()))
            mid = oracle_mod.warp_blend(frames_np[k], frames_np[k + 1], None, 0.5, threads=0)
            want = oracle_mod.lanczos3(mid, 2 * w, 2 * h, threads=0).astype(np.int16)
            d = np.abs(fetch(fused[k]).astype(np.int16) - want)
            assert d.max() <= 1 and (d > 0).mean() < 1e-3, (pattern, "fused", k, int(d.max()), float((d > 0).mean()))
        del frames, out, fused


def test_config3_1080p_interpolation(nsc, oracle_mod):
    a = oracle_mod.gen_gradient(1920, 1080, 0)
    b = oracle_mod.gen_gradient(1920, 1080, 1)
    it = nsc.WgpuFrameInterpolator()
    out = np.frombuffer(it.interpolate_py(a.tobytes(), b.tobytes(), 1920, 1080, time_t=0.5), np.uint8).reshape(1080, 1920, 4)
    want = oracle_mod.warp_blend(a, b, None, 0.5, threads=0)
    assert _maxdiff(out, want) <= 1 and np.array_equal(out, want)
    flow = np.zeros((1080, 1920, 2), np.float32)
    flow[..., 0] = -1.0
    out = np.frombuffer(it.interpolate_py(a.tobytes(), b.tobytes(), 1920, 1080, time_t=0.5, flow=flow), np.uint8).reshape(1080, 1920, 4)
    assert np.array_equal(out, oracle_mod.warp_blend(a, b, flow, 0.5, threads=0))
    # idempotence at the end points
    assert it.interpolate_py(a.tobytes(), b.tobytes(), 1920, 1080, time_t=0.0) == a.tobytes()
    assert it.interpolate_py(a.tobytes(), b.tobytes(), 1920, 1080, time_t=1.0) == b.tobytes()


def test_swizzle_bgra_to_rgba_device(nsc, oracle_mod):
    import torch

    for n in (64 * 36, 61 * 7):  # vector and scalar paths
        bgra = put(oracle_mod.gen_noise(n, 1, 77).reshape(n, 4).copy())
        out = guarded.empty_like(bgra)
        nsc.swizzle_bgra_to_rgba_device(bgra.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(fetch(out), fetch(bgra)[:, [2, 1, 0, 3]])
        nsc.swizzle_bgra_to_rgba_device(out.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)  # in place
        torch.cuda.synchronize()
        assert np.array_equal(fetch(out), fetch(bgra))


@pytest.mark.parametrize("alg", ["lanczos3", "bicubic"])
@pytest.mark.parametrize("t", [0.5, 0.3, 0.0, 1.0])
def test_fused_blend_upscale_equals_two_stage(nsc, oracle_mod, alg, t):
    """upscale_blend_device == interpolate (zero flow) then upscale, bit for bit (sliding stream layout)."""
    import torch

    w, h, n = 128, 40, 4
    dev = torch.device("cuda:0")
    frames_np = np.stack([oracle_mod.gen_noise(w, h, 300 + i) for i in range(n + 1)])
    frames = put(frames_np)
    filt = {"lanczos3": 0, "bicubic": 1}[alg]
    for mode in ("exact", "fma"):
        u = nsc.PyWgpuUpscaler("quality", alg, lanczos_mode=mode)
        u.initialize(w, h, 2 * w, 2 * h)
        fused = guarded.zeros((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device=dev)
        fb = w * h * 4
        u.upscale_blend_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, t, fused.data_ptr(), n,
                               torch.cuda.current_stream().cuda_stream)
        # two-stage reference on the GPU
        it = nsc.WgpuFrameInterpolator()
        mid = guarded.empty((n, h, w, 4), dtype=torch.uint8, device=dev)
        two = guarded.zeros_like(fused)
        s = torch.cuda.current_stream().cuda_stream
        it.interpolate_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, 0, w, h, t, mid.data_ptr(), n, s)
        u.upscale_device(mid.data_ptr(), two.data_ptr(), n, s)
        torch.cuda.synchronize()
        assert torch.equal(fused, two), (alg, t, mode)
        if mode == "exact":
            for i in range(n):
                m = oracle_mod.warp_blend(frames_np[i], frames_np[i + 1], None, t)
                assert np.array_equal(fetch(fused[i]), oracle_mod.resize(m, 2 * w, 2 * h, filt)), (alg, t, i)
        if mode == "fma":
            for i in range(n):
                m = oracle_mod.warp_blend(frames_np[i], frames_np[i + 1], None, t)
                check_fma(oracle_mod, fetch(fused[i]), m, 2 * w, 2 * h, filt, (alg, t, i, u.kernel_variant))
    ub = nsc.PyWgpuUpscaler("quality", "bilinear")
    ub.initialize(w, h, 2 * w, 2 * h)
    with pytest.raises(RuntimeError, match="only the exact-x2 resize kernels"):
        ub.upscale_blend_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, 0.5, fused.data_ptr(), 1, 0)


def test_concurrent_calls_on_one_handle_are_serialised(nsc, oracle_mod):
    """The reference calls upscale(&self) from rayon threads (upscale/mod.rs:619-624): one handle,
    many threads.  ctypes releases the GIL, so these really run concurrently into the C ABI."""
    import threading

    w, h = 96, 40
    u = nsc.PyWgpuUpscaler("quality", "lanczos3", lanczos_mode="exact")
    u.initialize(w, h, 2 * w, 2 * h)
    frames = [oracle_mod.gen_noise(w, h, 500 + i) for i in range(8)]
    want = [oracle_mod.lanczos3(f, 2 * w, 2 * h) for f in frames]
    got, errs = [None] * len(frames), []

    def work(i):
        try:
            for _ in range(5):
                got[i] = np.frombuffer(u.upscale(frames[i].tobytes()), np.uint8).reshape(2 * h, 2 * w, 4)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(frames))]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errs
    for g, wnt in zip(got, want):
        assert np.array_equal(g, wnt)


def test_device_path_is_graph_capturable(nsc, oracle_mod):
    """The device entry points allocate nothing and never synchronise: one pipeline step can be
    captured into a hipGraph and replayed."""
    import torch

    w, h, n = 128, 24, 3
    dev = torch.device("cuda:0")
    frames_np = np.stack([oracle_mod.gen_noise(w, h, 600 + i) for i in range(n + 1)])
    frames = put(frames_np)
    pipe = nsc.FramePipeline(w, h, 2, "lanczos3", 0.5, lanczos_mode="exact")
    mid, up_real, up_mid = guarded.like(pipe.alloc(n, dev))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pipe.step(frames, mid, up_real, up_mid, side.cuda_stream)  # warm-up outside capture
    side.synchronize()
    for t in (mid, up_real, up_mid):
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pipe.step(frames, mid, up_real, up_mid, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(up_real.max()) == 0  # capture does not execute
    g.replay()
    torch.cuda.synchronize()
    for i in range(n):
        m = oracle_mod.warp_blend(frames_np[i], frames_np[i + 1], None, 0.5)
        assert np.array_equal(fetch(mid[i]), m)
        assert np.array_equal(fetch(up_real[i]), oracle_mod.lanczos3(frames_np[i], 2 * w, 2 * h))
        assert np.array_equal(fetch(up_mid[i]), oracle_mod.lanczos3(m, 2 * w, 2 * h))


# ---- BGRA input: the capture feed's channel order, swizzled inside the kernels' loads ----------

def _bgra(img):
    return np.ascontiguousarray(img[..., [2, 1, 0, 3]])


@pytest.mark.parametrize("alg,kw", [("nearest", {}), ("bilinear", {}), ("bilinear", {"bilinear_variant": "wgsl"}),
                                    ("lanczos3", {}), ("lanczos3", {"lanczos_mode": "exact"}), ("bicubic", {}),
                                    ("triangle", {}), ("fsr1", {}), ("easu", {})])
@pytest.mark.parametrize("dims,opts", [(((252, 40), (504, 80)), {}), (((252, 40), (504, 80)), {"force_general": 1}),
                                       (((252, 40), (504, 80)), {"force_general": 1, "force_rows": 1}),
                                       (((48, 27), (72, 41)), {}), (((64, 36), (128, 72)), {"force_per_pixel": 1, "force_general": 1}),
                                       (((100, 40), (30, 12)), {})])
def test_bgra_input_equals_swizzle_then_upscale(nsc, oracle_mod, alg, kw, dims, opts):
    """Upscaling a BGRA frame with input format "bgra" == upscaling its RGBA swizzle, for every kernel variant."""
    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 41)
    want, u0 = _up(nsc, alg, img, ow, oh, options=dict(opts), **kw)
    u = nsc.PyWgpuUpscaler("quality", alg, **kw)
    for k, v in opts.items():
        u.set_option(k, v)
    u.set_input_format("bgra")
    u.initialize(w, h, ow, oh)
    got = np.frombuffer(u.upscale(_bgra(img).tobytes()), np.uint8).reshape(oh, ow, 4)
    assert u.kernel_variant == u0.kernel_variant
    assert np.array_equal(got, want), (alg, u.kernel_variant)
    u.set_input_format("rgba")  # switchable at any time
    assert np.array_equal(np.frombuffer(u.upscale(img.tobytes()), np.uint8).reshape(oh, ow, 4), want)
    with pytest.raises(ValueError):
        u.set_input_format("argb")


def test_bgra_input_interpolator_and_fused_blend(nsc, oracle_mod):
    import torch
    w, h = 252, 40
    a, b = oracle_mod.gen_noise(w, h, 42), oracle_mod.gen_noise(w, h, 43)
    flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = 1.25, -0.5
    it = nsc.WgpuFrameInterpolator()
    it.set_input_format("bgra")
    for f in (None, flow):
        for t in (0.5, 0.3):
            got = np.frombuffer(it.interpolate_py(_bgra(a).tobytes(), _bgra(b).tobytes(), w, h, time_t=t, flow=f), np.uint8)
            assert np.array_equal(got.reshape(h, w, 4), oracle_mod.warp_blend(a, b, f, t))
    # fused blend + x2 upscale on BGRA pairs
    for alg in ("lanczos3", "bicubic"):
        for t in (0.5, 0.3):
            u = nsc.PyWgpuUpscaler("quality", alg)
            u.initialize(w, h, 2 * w, 2 * h)
            mid = oracle_mod.warp_blend(a, b, None, t)
            want = np.frombuffer(u.upscale(mid.tobytes()), np.uint8).reshape(2 * h, 2 * w, 4)
            u.set_input_format("bgra")
            da, db = put(_bgra(a)), put(_bgra(b))
            out = guarded.empty((2 * h, 2 * w, 4), dtype=torch.uint8, device="cuda")
            u.upscale_blend_device(da.data_ptr(), 0, db.data_ptr(), 0, t, out.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(fetch(out), want), (alg, t)


# ---- seeded random shape sweep: ragged widths around the kernels' segment sizes --------------------

def _random_dims(seed, n):
    rng = np.random.default_rng(seed)
    dims = []
    for _ in range(n):
        w = int(rng.choice([rng.integers(1, 40), rng.integers(60, 70), rng.integers(120, 135), rng.integers(250, 262),
                            rng.integers(505, 520)]))
        h = int(rng.integers(1, 48))
        kind = rng.integers(0, 4)
        if kind == 0:  # exact x2
            ow, oh = 2 * w, 2 * h
        elif kind == 1:  # any up-scale, independent per axis
            ow, oh = int(w * rng.uniform(1.0, 3.2)) + 1, int(h * rng.uniform(1.0, 3.2)) + 1
        elif kind == 2:  # down-scale (kept within the 32-tap window of the resize filters)
            ow, oh = max(1, int(w / rng.uniform(1.0, 3.0))), max(1, int(h / rng.uniform(1.0, 3.0)))
        else:  # mixed
            ow, oh = int(w * rng.uniform(1.0, 2.5)) + 1, max(1, int(h / rng.uniform(1.0, 2.5)))
        dims.append(((w, h), (ow, oh)))
    return dims


@pytest.mark.parametrize("alg", ["nearest", "bilinear", "lanczos3", "bicubic", "triangle", "fsr1"])
def test_random_shape_sweep(nsc, oracle_mod, alg):
    ref = {"nearest": oracle_mod.nearest, "bilinear": oracle_mod.bilinear,
           "lanczos3": lambda i, ow, oh: oracle_mod.resize(i, ow, oh, oracle_mod.FILTER_LANCZOS3),
           "bicubic": lambda i, ow, oh: oracle_mod.resize(i, ow, oh, oracle_mod.FILTER_CATMULLROM),
           "triangle": lambda i, ow, oh: oracle_mod.resize(i, ow, oh, oracle_mod.FILTER_TRIANGLE),
           "fsr1": lambda i, ow, oh: oracle_mod.fsr1(i, ow, oh, 0.0, 0.7)}[alg]
    resize = alg in ("lanczos3", "bicubic", "triangle")
    seen = set()
    seed = {"nearest": 1, "bilinear": 2, "lanczos3": 3, "bicubic": 4, "triangle": 5, "fsr1": 6}[alg]
    for k, ((w, h), (ow, oh)) in enumerate(_random_dims(seed, 40)):
        img = oracle_mod.gen_noise(w, h, 100 + k)
        want = ref(img, ow, oh)
        if resize:
            got, u = _up(nsc, alg, img, ow, oh, lanczos_mode="exact")
            assert np.array_equal(got, want), (alg, (w, h), (ow, oh), u.kernel_variant)
            got_f, _ = _up(nsc, alg, img, ow, oh)
            assert _maxdiff(got_f, want) <= 1, (alg, (w, h), (ow, oh))
            check_fma(oracle_mod, got_f, img, ow, oh, {"lanczos3": 0, "bicubic": 1, "triangle": 2}[alg],
                      (alg, (w, h), (ow, oh), u.kernel_variant))
        else:
            got, u = _up(nsc, alg, img, ow, oh)
            assert np.array_equal(got, want), (alg, (w, h), (ow, oh), u.kernel_variant)
        seen.add(u.kernel_variant)
    assert len(seen) >= (2 if alg != "fsr1" else 1), seen


@pytest.mark.parametrize("alg", ["lanczos3", "bicubic"])
def test_lanczos_x2_opaque_and_mixed_alpha_rows(nsc, oracle_mod, alg):
    """The x2 kernel drops to 3 channels where the whole tap window of a wave is opaque; frames that are
    opaque, opaque in bands, or opaque except for single pixels must all match the 4-channel result."""
    filt = oracle_mod.FILTER_LANCZOS3 if alg == "lanczos3" else oracle_mod.FILTER_CATMULLROM
    w, h = 520, 90  # three strips wide (two full + a ragged one), a few row blocks tall
    base = oracle_mod.gen_noise(w, h, 77)
    variants = {}
    v = base.copy(); v[..., 3] = 255; variants["opaque"] = v
    v = base.copy(); v[..., 3] = 255; v[20:27, :, 3] = base[20:27, :, 3]; variants["band"] = v
    v = base.copy(); v[..., 3] = 255; v[40, 300, 3] = 254; v[0, 0, 3] = 0; v[h - 1, w - 1, 3] = 17; variants["pixels"] = v
    v = base.copy(); v[..., 3] = 255; v[:, 248:256, 3] = 7; variants["strip_seam"] = v
    for name, img in variants.items():
        want = oracle_mod.resize(img, 2 * w, 2 * h, filt)
        got, u = _up(nsc, alg, img, 2 * w, 2 * h)
        assert u.kernel_variant == "lanczos3_x2_regwin"
        assert _maxdiff(got, want) <= 1, name
        check_fma(oracle_mod, got, img, 2 * w, 2 * h, filt, (alg, name))
        opaque_out = want[..., 3] == 255  # wherever the CPU says 255, so must the GPU (constant or 4-channel path)
        if name == "opaque":
            assert opaque_out.all() and (got[..., 3] == 255).all()
        # away from the non-opaque pixels' 6-tap footprint the 3-channel path wrote the constant
        far = np.ones((2 * h, 2 * w), bool)
        ys, xs = np.nonzero(img[..., 3] != 255)
        for y, x in zip(ys.tolist(), xs.tolist()):
            far[max(0, 2 * y - 8):2 * y + 10, max(0, 2 * x - 8):2 * x + 10] = False
        assert (got[..., 3][far] == 255).all() and (want[..., 3][far] == 255).all(), name
        got_e, _ = _up(nsc, alg, img, 2 * w, 2 * h, lanczos_mode="exact")
        assert np.array_equal(got_e, want), name


@pytest.mark.parametrize("alg", ["lanczos3", "bicubic"])
def test_lanczos_x2_flat_alpha_windows_take_the_three_channel_path(nsc, oracle_mod, alg):
    """Round 5: the 3-channel path of the x2 kernel is taken wherever the alpha of a wave's 6-row window is ONE value -- any value,
    not only 255 (overlays with alpha 0 / 17 / 128, a band of another alpha across all rows, mixed rows).  Three proofs:
      * against the oracle: every sample within 1 LSB, < 0.1 % different (the FMA contract), and the ALPHA channel equal to the
        oracle's wherever the whole window is flat (the constant is what the CPU computes: taps are normalised);
      * against the 4-channel path: the same frame with one alpha bit flipped in every (row, strip) -- no window is flat any more,
        every wave takes the 4-channel path -- gives bit-identical R, G, B everywhere (channels never mix) and bit-identical alpha
        outside the flipped pixels' tap footprints: where both paths computed an alpha, they computed the same byte;
      * EXACT mode (no 3-channel path at all) equals the oracle bit for bit on the same frames."""
    filt = oracle_mod.FILTER_LANCZOS3 if alg == "lanczos3" else oracle_mod.FILTER_CATMULLROM
    w, h = 1000, 104  # five strips (four full + a ragged one), several row blocks
    img = oracle_mod.gen_noise(w, h, 4242)
    img[0:40, :, 3] = 255
    img[40:60, :, 3] = 128
    img[60:83, :, 3] = 17
    img[83:, :, 3] = 0
    img[:, 500:700, 3] = 200      # a band of another alpha down all rows: strips that straddle its borders are not flat
    img[50, :, 3] = 129           # one row of its own inside a region: windows that hold it and its neighbours are mixed
    rowwise = img.copy()
    rowwise[:, :, 3] = (np.arange(h, dtype=np.uint8) * 3)[:, None]  # every row flat, no two rows alike: never six in a row
    for name, frame in (("regions", img), ("rowwise", rowwise)):
        want = oracle_mod.resize(frame, 2 * w, 2 * h, filt, threads=0)
        got, u = _up(nsc, alg, frame, 2 * w, 2 * h, options={"rows_per_wave": 26})
        assert u.kernel_variant == "lanczos3_x2_regwin"
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3, (name, int(d.max()), float((d > 0).mean()))
        # flat windows: input alpha constant over rows y-3 .. y+3 and columns x-3 .. x+3 => both CPU and GPU say that constant
        a = frame[..., 3].astype(np.int16)
        flat = np.ones((h, w), bool)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                sh = np.roll(np.roll(a, dy, 0), dx, 1)
                flat &= sh == a
        flat[:3] = flat[-3:] = False
        flat[:, :3] = flat[:, -3:] = False
        up_flat = np.repeat(np.repeat(flat, 2, 0), 2, 1)
        up_a = np.repeat(np.repeat(frame[..., 3], 2, 0), 2, 1)
        assert np.array_equal(want[..., 3][up_flat], up_a[up_flat]) and np.array_equal(got[..., 3][up_flat], up_a[up_flat]), name
        if name == "regions":
            assert up_flat.mean() > 0.5
        # the same frame through the 4-channel path everywhere
        broken = frame.copy()
        xs = [s_ * 240 + 7 for s_ in range((w + 239) // 240)]
        for x in xs:
            broken[:, x, 3] ^= 1
        got4, _ = _up(nsc, alg, broken, 2 * w, 2 * h, options={"rows_per_wave": 26})
        assert np.array_equal(got[..., :3], got4[..., :3]), name
        near = np.zeros((2 * h, 2 * w), bool)
        for x in xs:
            near[:, max(0, 2 * x - 8):2 * x + 10] = True
        assert np.array_equal(got[..., 3][~near], got4[..., 3][~near]), name
        got_e, _ = _up(nsc, alg, frame, 2 * w, 2 * h, lanczos_mode="exact")
        assert np.array_equal(got_e, want), name


@pytest.mark.parametrize("alg,filt", [("lanczos3", 0), ("bicubic", 1), ("triangle", 2)])
@pytest.mark.parametrize("dims", [((320, 180), (480, 270)), ((320, 180), (960, 540)), ((250, 135), (1000, 540)),
                                  ((640, 360), (960, 540)), ((100, 37), (1000, 99)), ((480, 270), (680, 384)), ((600, 40), (900, 41)),
                                  ((480, 270), (640, 360)), ((517, 40), (520, 41)), ((1000, 30), (1200, 36)),
                                  ((255, 33), (1020, 200)), ((64, 64), (64, 64))])
def test_resize_register_window_variant(nsc, oracle_mod, alg, filt, dims):
    """Up-scaling shapes (x1 .. x10, ow % 4 == 0) take the register-window variant; it must equal the LDS-row
    variant bit for bit in both modes, and the oracle in EXACT mode."""
    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 91)
    want = oracle_mod.resize(img, ow, oh, filt)
    # exact x3, x3/2 and x4/3 have their own kernels: ask for this one
    gen = {"force_general": 1} if (ow, oh) == (3 * w, 3 * h) or (2 * ow, 2 * oh) == (3 * w, 3 * h) or (3 * ow, 3 * oh) == (4 * w, 4 * h) else {}
    if any((q * ow, q * oh) == (p * w, p * h) for p, q in ((5, 4), (6, 5), (5, 3), (5, 2), (7, 2), (7, 5), (8, 5), (9, 5))):
        gen = {"force_general": 1}  # (these factors have the P/Q kernel since round 5)
    got_e, u = _up(nsc, alg, img, ow, oh, lanczos_mode="exact", options=dict(gen))
    assert u.kernel_variant == "resize_regwin_lds"
    assert np.array_equal(got_e, want)
    got_f, _ = _up(nsc, alg, img, ow, oh, options=dict(gen))
    ref_f, ur = _up(nsc, alg, img, ow, oh, options=dict(gen, force_rows=1))
    assert ur.kernel_variant == "resize_rows_lds"
    assert np.array_equal(got_f, ref_f) and _maxdiff(got_f, want) <= 1
    check_fma(oracle_mod, got_f, img, ow, oh, filt, (alg, dims, u.kernel_variant, gen))


@pytest.mark.parametrize("alg,filt", [("lanczos3", 0), ("bicubic", 1), ("triangle", 2)])
@pytest.mark.parametrize("factor", [3, 4])
@pytest.mark.parametrize("size", [(64, 36), (252, 20), (256, 33), (16, 16), (500, 17), (1000, 50), (248, 40), (496, 19)])
def test_resize_integer_factor_register_window(nsc, oracle_mod, alg, filt, factor, size):
    """x3 / x4 (720p -> 4K, 540p -> 4K): the x2 kernel's register-window design with S rows per input row."""
    w, h = size
    ow, oh = factor * w, factor * h
    img = oracle_mod.gen_noise(w, h, 93)
    want = oracle_mod.resize(img, ow, oh, filt)
    got_e, u = _up(nsc, alg, img, ow, oh, lanczos_mode="exact")
    # x4: one set of interior weights per phase.  x3: (o + 0.5) * fl(1/3) is rounded in f32, so the weights move with
    # the binade of the coordinate; the host groups the input indices into weight classes and every lane / row of
    # the same kernel takes the set of its class (exact: EXACT mode stays at 0 differences).
    assert u.kernel_variant == "lanczos3_xs_regwin"
    assert np.array_equal(got_e, want)
    got_f, uf = _up(nsc, alg, img, ow, oh)
    assert uf.kernel_variant == "lanczos3_xs_regwin"
    # FMA mode packs with round-to-nearest-even; Triangle's dyadic weights put many sums on exact .5 ties,
    # where that differs from f32::round by one count
    assert _maxdiff(got_f, want) <= 1 and (got_f != want).mean() < (3e-2 if alg == "triangle" else 1e-3)
    check_fma(oracle_mod, got_f, img, ow, oh, filt, (alg, factor, size, uf.kernel_variant))  # (Triangle: ties)
    # the general kernels agree (same weights, same operation order)
    ref_e, ug = _up(nsc, alg, img, ow, oh, lanczos_mode="exact", options={"force_general": 1})
    assert ug.kernel_variant in ("resize_regwin_lds", "resize_rows_lds") and np.array_equal(ref_e, want)
    for th in (1, 7, 24):
        out_t, _ = _up(nsc, alg, img, ow, oh, lanczos_mode="exact", options={"rows_per_wave": th})
        assert np.array_equal(out_t, want), th
    # BGRA input
    ub = nsc.PyWgpuUpscaler("quality", alg, lanczos_mode="exact")
    ub.set_input_format("bgra")
    ub.initialize(w, h, ow, oh)
    got_b = np.frombuffer(ub.upscale(_bgra(img).tobytes()), np.uint8).reshape(oh, ow, 4)
    assert np.array_equal(got_b, want)


@pytest.mark.parametrize("alg,filt", [("lanczos3", 0), ("bicubic", 1), ("triangle", 2)])
@pytest.mark.parametrize("size", [(64, 36), (32, 16), (256, 34), (248, 40), (496, 18), (480, 270), (1000, 50), (744, 22)])
def test_resize_factor_three_halves_register_window(nsc, oracle_mod, alg, filt, size):
    """x3/2 (720p -> 1080p, 1440p -> 4K): the register-window design with three output rows per pair of input rows and
    three horizontal phases per pair of columns; weights per class of the input pair (they move with the binade of the
    sample coordinate).  EXACT mode: 0 differences; FMA mode: the bits of the general kernel (same order of operations)."""
    w, h = size
    ow, oh = 3 * w // 2, 3 * h // 2
    img = oracle_mod.gen_noise(w, h, 95)
    want = oracle_mod.resize(img, ow, oh, filt)
    got_e, u = _up(nsc, alg, img, ow, oh, lanczos_mode="exact")
    assert u.kernel_variant == "lanczos3_r32_regwin"
    assert np.array_equal(got_e, want)
    got_f, uf = _up(nsc, alg, img, ow, oh)
    assert uf.kernel_variant == "lanczos3_r32_regwin"
    # FMA mode packs with round-to-nearest-even; Triangle's weights put many sums on exact .5 ties (see the x3 / x4 test)
    assert _maxdiff(got_f, want) <= 1 and (got_f != want).mean() < (5e-2 if alg == "triangle" else 1e-3)
    check_fma(oracle_mod, got_f, img, ow, oh, filt, (alg, (w, h), (ow, oh), uf.kernel_variant))  # (Triangle: ties)
    ref_f, ug = _up(nsc, alg, img, ow, oh, options={"force_general": 1})
    assert ug.kernel_variant in ("resize_regwin_lds", "resize_rows_lds") and np.array_equal(got_f, ref_f)
    for th in (2, 6, 24, 37):
        out_t, _ = _up(nsc, alg, img, ow, oh, lanczos_mode="exact", options={"rows_per_wave": th})
        assert np.array_equal(out_t, want), th
    # opaque frames (the 3-channel path) and BGRA input
    opq = img.copy()
    opq[..., 3] = 255
    got_o, _ = _up(nsc, alg, opq, ow, oh)
    ref_o, _ = _up(nsc, alg, opq, ow, oh, options={"force_general": 1})
    assert np.array_equal(got_o, ref_o) and (got_o[..., 3] == 255).all()
    ub = nsc.PyWgpuUpscaler("quality", alg, lanczos_mode="exact")
    ub.set_input_format("bgra")
    ub.initialize(w, h, ow, oh)
    got_b = np.frombuffer(ub.upscale(_bgra(img).tobytes()), np.uint8).reshape(oh, ow, 4)
    assert np.array_equal(got_b, want)


@pytest.mark.parametrize("alg,filt", [("lanczos3", 0), ("bicubic", 1), ("triangle", 2)])
@pytest.mark.parametrize("size", [(48, 18), (96, 36), (192, 21), (372, 33), (384, 45), (564, 24), (960, 54), (1116, 30)])
def test_resize_factor_four_thirds_register_window(nsc, oracle_mod, alg, filt, size):
    """x4/3 (1080p -> 1440p): four output rows per group of three input rows, four phases per group of three columns, one lane
    per column group (12 bytes in, 16 contiguous bytes out); the ratio 3/4 is exact in f32, so one set of weights per phase.
    EXACT mode: 0 differences; FMA mode: the bits of the general kernel."""
    w, h = size
    ow, oh = 4 * w // 3, 4 * h // 3
    img = oracle_mod.gen_noise(w, h, 96)
    want = oracle_mod.resize(img, ow, oh, filt)
    got_e, u = _up(nsc, alg, img, ow, oh, lanczos_mode="exact")
    assert u.kernel_variant == "lanczos3_r43_regwin"
    assert np.array_equal(got_e, want)
    got_f, uf = _up(nsc, alg, img, ow, oh)
    assert uf.kernel_variant == "lanczos3_r43_regwin"
    assert _maxdiff(got_f, want) <= 1 and (got_f != want).mean() < (5e-2 if alg == "triangle" else 1e-3)
    check_fma(oracle_mod, got_f, img, ow, oh, filt, (alg, (w, h), (ow, oh), uf.kernel_variant))  # (Triangle: ties)
    ref_f, ug = _up(nsc, alg, img, ow, oh, options={"force_general": 1})
    assert ug.kernel_variant in ("resize_regwin_lds", "resize_rows_lds") and np.array_equal(got_f, ref_f)
    for th in (3, 7, 24, 40):
        out_t, _ = _up(nsc, alg, img, ow, oh, lanczos_mode="exact", options={"rows_per_wave": th})
        assert np.array_equal(out_t, want), th
    opq = img.copy()
    opq[..., 3] = 255
    got_o, _ = _up(nsc, alg, opq, ow, oh)
    ref_o, _ = _up(nsc, alg, opq, ow, oh, options={"force_general": 1})
    assert np.array_equal(got_o, ref_o) and (got_o[..., 3] == 255).all()
    ub = nsc.PyWgpuUpscaler("quality", alg, lanczos_mode="exact")
    ub.set_input_format("bgra")
    ub.initialize(w, h, ow, oh)
    got_b = np.frombuffer(ub.upscale(_bgra(img).tobytes()), np.uint8).reshape(oh, ow, 4)
    assert np.array_equal(got_b, want)


_PQ_SIZES = {(5, 4): [(32, 12), (64, 36), (240, 40), (252, 20), (496, 24), (1008, 48), (1120, 32)],
             (6, 5): [(40, 15), (310, 20), (320, 25), (620, 30), (1000, 50)],
             (5, 3): [(36, 12), (180, 21), (189, 33), (372, 18), (960, 54)],
             (5, 2): [(32, 12), (120, 20), (122, 14), (240, 30), (600, 40)],
             (7, 2): [(32, 12), (120, 20), (126, 14), (248, 30)],
             (7, 5): [(40, 15), (300, 20), (620, 30)],
             (8, 5): [(35, 15), (315, 25), (1000, 50)],
             (9, 5): [(40, 15), (300, 20), (620, 30)]}


@pytest.mark.parametrize("alg,filt", [("lanczos3", 0), ("bicubic", 1), ("triangle", 2)])
@pytest.mark.parametrize("factor,size", [(f, sz) for f, sizes in _PQ_SIZES.items() for sz in sizes])
def test_resize_small_rational_factor_register_window(nsc, oracle_mod, alg, filt, factor, size):
    """x5/4, x6/5, x7/5, x8/5, x9/5, x5/3, x5/2, x7/2 (the reference's scale slider moves in tenths: nu_scaler_py/nu_scaler/main.py:457-459): P output rows per
    group of Q input rows, one lane per group of Q columns, every output's weights from the tables in frame form (the ratios are not
    exact in f32).  EXACT mode: 0 differences from the oracle; FMA mode: the bits of the general kernel; borders, strip joints
    (widths around the strips of 62 Q / 60 Q columns), any number of rows per wave, opaque rows, BGRA input.  Output widths that are
    not a multiple of 4 (252 -> 315, 189 -> 315, 122 -> 305, 126 -> 441) keep the any-scale kernel."""
    P, Q = factor
    w, h = size
    ow, oh = P * w // Q, P * h // Q
    img = oracle_mod.gen_noise(w, h, 97)
    want = oracle_mod.resize(img, ow, oh, filt)
    got_e, u = _up(nsc, alg, img, ow, oh, lanczos_mode="exact")
    # (the kernel stores whole 16-byte pieces of the output row: widths that are not a multiple of 4 keep the any-scale kernels)
    kernel = "lanczos3_pq_regwin" if ow % 4 == 0 else "resize_rows_lds"
    assert u.kernel_variant == kernel
    assert np.array_equal(got_e, want)
    got_f, uf = _up(nsc, alg, img, ow, oh)
    assert uf.kernel_variant == kernel
    assert _maxdiff(got_f, want) <= 1 and (got_f != want).mean() < (5e-2 if alg == "triangle" else 1e-3)
    check_fma(oracle_mod, got_f, img, ow, oh, filt, (alg, (w, h), (ow, oh), uf.kernel_variant))  # (Triangle: ties)
    ref_f, ug = _up(nsc, alg, img, ow, oh, options={"force_general": 1})
    assert ug.kernel_variant in ("resize_regwin_lds", "resize_rows_lds") and np.array_equal(got_f, ref_f)
    if kernel == "lanczos3_pq_regwin":
        # round 6: a support-2 (Catmull-Rom) or support-1 (Triangle) filter leaves slots 0 and 5 of every 6-slot frame zero, and the
        # kernel then sums 4 taps per pass (NARROW): the very bytes of the 6-tap form, in both modes (v * 0 changes no sum)
        assert (uf.get_option("pq_p"), uf.get_option("pq_q")) == (P, Q)
        assert uf.get_option("pq_narrow_active") == (0 if alg == "lanczos3" else 1)
        if alg != "lanczos3":
            six_f, u6 = _up(nsc, alg, img, ow, oh, options={"pq_narrow": 0})
            assert u6.get_option("pq_narrow_active") == 0 and u6.kernel_variant == kernel and np.array_equal(six_f, got_f)
            six_e, _ = _up(nsc, alg, img, ow, oh, lanczos_mode="exact", options={"pq_narrow": 0})
            assert np.array_equal(six_e, got_e)
    for th in (Q, 7, 24, 40):
        out_t, _ = _up(nsc, alg, img, ow, oh, lanczos_mode="exact", options={"rows_per_wave": th})
        assert np.array_equal(out_t, want), th
    opq = img.copy()
    opq[..., 3] = 255
    got_o, _ = _up(nsc, alg, opq, ow, oh)
    ref_o, _ = _up(nsc, alg, opq, ow, oh, options={"force_general": 1})
    assert np.array_equal(got_o, ref_o) and (got_o[..., 3] == 255).all()
    band = opq.copy()
    band[h // 2:h // 2 + 2, :, 3] = img[h // 2:h // 2 + 2, :, 3]
    got_m, _ = _up(nsc, alg, band, ow, oh)
    ref_m, _ = _up(nsc, alg, band, ow, oh, options={"force_general": 1})
    assert np.array_equal(got_m, ref_m)
    ub = nsc.PyWgpuUpscaler("quality", alg, lanczos_mode="exact")
    ub.set_input_format("bgra")
    ub.initialize(w, h, ow, oh)
    got_b = np.frombuffer(ub.upscale(_bgra(img).tobytes()), np.uint8).reshape(oh, ow, 4)
    assert np.array_equal(got_b, want)


@pytest.mark.parametrize("dims", [((1536, 864), (1920, 1080)), ((1600, 900), (1920, 1080)), ((1920, 1080), (3200, 1800)),
                                  ((1536, 864), (3840, 2160))])
def test_small_rational_factors_at_full_size(nsc, oracle_mod, dims):
    """864p / 900p -> 1080p, 1080p -> 1800p, 864p -> 4K at full size: both modes against the oracle, and a device batch against the
    single frames."""
    import torch

    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 98)
    want = oracle_mod.lanczos3(img, ow, oh, threads=0)
    got_f, uf = _up(nsc, "lanczos3", img, ow, oh)
    assert uf.kernel_variant == "lanczos3_pq_regwin"
    d = np.abs(got_f.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    got_e, ue = _up(nsc, "lanczos3", img, ow, oh, lanczos_mode="exact")
    assert ue.kernel_variant == "lanczos3_pq_regwin" and np.array_equal(got_e, want)
    frames = np.stack([img, img[::-1].copy(), oracle_mod.gen_gradient(w, h)])
    d_in = put(frames)
    d_out = guarded.empty((3, oh, ow, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    uf.upscale_device(d_in.data_ptr(), d_out.data_ptr(), 3)
    torch.cuda.synchronize()
    got_b = fetch(d_out)
    assert np.array_equal(got_b[0], got_f)
    for k in (1, 2):
        single, _ = _up(nsc, "lanczos3", frames[k], ow, oh)
        assert np.array_equal(got_b[k], single), k


def test_1080p_to_1440p_takes_the_four_thirds_kernel(nsc, oracle_mod):
    w, h, ow, oh = 1920, 1080, 2560, 1440
    img = oracle_mod.gen_noise(w, h, 80)
    want = oracle_mod.lanczos3(img, ow, oh, threads=0)
    got_f, uf = _up(nsc, "lanczos3", img, ow, oh)
    assert uf.kernel_variant == "lanczos3_r43_regwin"
    d = np.abs(got_f.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    got_e, ue = _up(nsc, "lanczos3", img, ow, oh, lanczos_mode="exact")
    assert ue.kernel_variant == "lanczos3_r43_regwin" and np.array_equal(got_e, want)


def test_1440p_to_4k_takes_the_three_halves_kernel(nsc, oracle_mod):
    """2560x1440 -> 3840x2160 at full size, both modes against the oracle, and a device batch."""
    import torch

    w, h, ow, oh = 2560, 1440, 3840, 2160
    img = oracle_mod.gen_noise(w, h, 79)
    want = oracle_mod.lanczos3(img, ow, oh, threads=0)
    got_f, uf = _up(nsc, "lanczos3", img, ow, oh)
    assert uf.kernel_variant == "lanczos3_r32_regwin"
    d = np.abs(got_f.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    got_e, ue = _up(nsc, "lanczos3", img, ow, oh, lanczos_mode="exact")
    assert ue.kernel_variant == "lanczos3_r32_regwin" and np.array_equal(got_e, want)
    n = 3
    frames_np = np.stack([oracle_mod.gen_gradient(w, h, k) for k in range(n)])
    frames = put(frames_np)
    out = guarded.zeros((n, oh, ow, 4), dtype=torch.uint8, device="cuda:0")
    uf.upscale_device(frames.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ug = nsc.PyWgpuUpscaler("quality", "lanczos3")
    ug.set_option("force_general", 1)
    ug.initialize(w, h, ow, oh)
    assert ug.kernel_variant == "resize_regwin_lds"
    for k in range(n):
        got_k = fetch(out[k])
        wk = oracle_mod.lanczos3(frames_np[k], ow, oh, threads=0).astype(np.int16)
        dk = np.abs(got_k.astype(np.int16) - wk)
        # the smooth gradient puts many sums of the FMA mode within a rounding of a .5 tie: more 1-LSB differences than on noise,
        # the same ones as the general kernel's (same order of operations)
        assert dk.max() <= 1 and (dk > 0).mean() < 1e-2, k
        ref_k = np.frombuffer(ug.upscale(frames_np[k].tobytes()), np.uint8).reshape(oh, ow, 4)
        assert np.array_equal(got_k, ref_k), k


def test_720p_to_4k_x3_takes_the_fixed_weight_kernel(nsc, oracle_mod):
    """The other headline resolution pair: 1280x720 -> 3840x2160 is exact x3.  Its weights are not uniform (they move
    with the binade of the sample coordinate), so the register-window kernel takes them per weight class; both
    modes against the oracle at full size, and a device batch."""
    import torch

    w, h, ow, oh = 1280, 720, 3840, 2160
    img = oracle_mod.gen_noise(w, h, 77)
    want = oracle_mod.lanczos3(img, ow, oh, threads=0)
    got_f, uf = _up(nsc, "lanczos3", img, ow, oh)
    assert uf.kernel_variant == "lanczos3_xs_regwin"
    d = np.abs(got_f.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    got_e, ue = _up(nsc, "lanczos3", img, ow, oh, lanczos_mode="exact")
    assert ue.kernel_variant == "lanczos3_xs_regwin" and np.array_equal(got_e, want)
    n = 3
    frames_np = np.stack([oracle_mod.gen_gradient(w, h, k) for k in range(n)])
    frames = put(frames_np)
    out = guarded.zeros((n, oh, ow, 4), dtype=torch.uint8, device="cuda:0")
    uf.upscale_device(frames.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k in range(n):
        wk = oracle_mod.lanczos3(frames_np[k], ow, oh, threads=0).astype(np.int16)
        dk = np.abs(fetch(out[k]).astype(np.int16) - wk)
        assert dk.max() <= 1 and (dk > 0).mean() < 1e-3, k


@pytest.mark.parametrize("alg", ["lanczos3", "bicubic", "fsr1", "bilinear", "nearest"])
@pytest.mark.parametrize("dims", [((64, 36), (256, 144)), ((64, 36), (96, 54)), ((64, 36), (192, 108)), ((96, 54), (64, 36))])
def test_device_batch_every_variant(nsc, oracle_mod, alg, dims):
    """n_frames > 1 through the device entry point (frames on the grid's z / y axis) for the x4, x1.5, x3 and
    down-scaling variants: each frame must equal the single-frame host result."""
    import torch
    (w, h), (ow, oh) = dims
    frames = np.stack([oracle_mod.gen_noise(w, h, 200 + k) for k in range(3)])
    u = nsc.PyWgpuUpscaler("quality", alg)
    u.initialize(w, h, ow, oh)
    want = [np.frombuffer(u.upscale(f.tobytes()), np.uint8).reshape(oh, ow, 4) for f in frames]
    d_in = put(frames)
    d_out = guarded.zeros((3, oh, ow, 4), dtype=torch.uint8, device="cuda")
    u.upscale_device(d_in.data_ptr(), d_out.data_ptr(), 3, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = fetch(d_out)
    for k in range(3):
        assert np.array_equal(got[k], want[k]), (alg, u.kernel_variant, k)


@pytest.mark.parametrize("alg,kw", [("nearest", {}), ("bilinear", {}), ("lanczos3", {}), ("lanczos3", {"lanczos_mode": "exact"}),
                                    ("bicubic", {}), ("fsr1", {})])
@pytest.mark.parametrize("dims", [((252, 40), (504, 80)), ((48, 27), (72, 41)), ((64, 36), (256, 144)), ((100, 40), (30, 12))])
@pytest.mark.parametrize("fmt", ["rgbx", "bgrx"])
def test_x_formats_read_alpha_as_opaque(nsc, oracle_mod, alg, kw, dims, fmt):
    """RGBX / BGRX: the alpha byte of the input is undefined and read as 255 inside the loads, so the result is
    the upscale of the opaque frame (and the x2 kernel takes its 3-channel path on every row)."""
    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 47)  # random alpha bytes: must be ignored
    opaque = img.copy()
    opaque[..., 3] = 255
    want, _ = _up(nsc, alg, opaque, ow, oh, **kw)
    u = nsc.PyWgpuUpscaler("quality", alg, **kw)
    u.set_input_format(fmt)
    u.initialize(w, h, ow, oh)
    src = img if fmt == "rgbx" else _bgra(img)
    got = np.frombuffer(u.upscale(src.tobytes()), np.uint8).reshape(oh, ow, 4)
    assert np.array_equal(got, want), (alg, fmt, u.kernel_variant)
    assert (got[..., 3] == 255).all()


def test_x_formats_interpolator(nsc, oracle_mod):
    w, h = 130, 33
    a, b = oracle_mod.gen_noise(w, h, 48), oracle_mod.gen_noise(w, h, 49)
    ao, bo = a.copy(), b.copy()
    ao[..., 3] = 255
    bo[..., 3] = 255
    flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0] = 0.75
    it = nsc.WgpuFrameInterpolator()
    it.set_input_format("bgrx")
    for f in (None, flow):
        got = np.frombuffer(it.interpolate_py(_bgra(a).tobytes(), _bgra(b).tobytes(), w, h, time_t=0.5, flow=f), np.uint8)
        assert np.array_equal(got.reshape(h, w, 4), oracle_mod.warp_blend(ao, bo, f, 0.5))


@pytest.mark.parametrize("alg", ["lanczos3", "bicubic"])
@pytest.mark.parametrize("dims", [((320, 180), (480, 270)), ((320, 90), (960, 270)), ((256, 64), (1024, 256))])
def test_resize_window_opaque_rows(nsc, oracle_mod, alg, dims):
    """Any-scale register-window kernel: output rows whose 7-row window is opaque in the wave skip alpha and store
    255; opaque, banded and single-pixel alpha must equal the LDS-row kernel (always 4 channels) bit for bit."""
    (w, h), (ow, oh) = dims
    base = oracle_mod.gen_noise(w, h, 78)
    variants = {}
    v = base.copy(); v[..., 3] = 255; variants["opaque"] = v
    v = base.copy(); v[..., 3] = 255; v[h // 2:h // 2 + 5, :, 3] = base[h // 2:h // 2 + 5, :, 3]; variants["band"] = v
    v = base.copy(); v[..., 3] = 255; v[h // 3, w // 2, 3] = 254; v[0, 0, 3] = 0; v[h - 1, w - 1, 3] = 9; variants["pixels"] = v
    for name, img in variants.items():
        got, u = _up(nsc, alg, img, ow, oh)
        assert u.kernel_variant in ("resize_regwin_lds", "lanczos3_xs_regwin", "lanczos3_r32_regwin", "lanczos3_r43_regwin", "lanczos3_pq_regwin")
        ref, ur = _up(nsc, alg, img, ow, oh, options={"force_general": 1, "force_rows": 1})
        assert ur.kernel_variant == "resize_rows_lds"
        assert np.array_equal(got, ref), name
        if name == "opaque":
            assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("alg,filt", [("lanczos3", 0), ("bicubic", 1), ("triangle", 2)])
@pytest.mark.parametrize("dims", [((256, 128), (128, 64)), ((300, 157), (150, 78)), ((515, 90), (172, 30)), ((640, 200), (160, 50)),
                                  ((200, 300), (133, 201)), ((130, 71), (129, 70)), ((97, 260), (61, 65)), ((70, 64), (33, 13)),
                                  ((64, 900), (16, 300)),
                                  # exactly 1/2 on both axes (4K -> 1080p's ratio), widths around the 64-output segments
                                  ((232, 60), (116, 30)), ((234, 62), (117, 31)), ((1000, 44), (500, 22)), ((116, 300), (58, 150))])
def test_resize_down_streaming_kernel(nsc, oracle_mod, alg, filt, dims):
    """Down-scaling (captured frames resized to the target, capture/common.rs:56): input rows streamed once into
    the vertical sums of the output rows in flight.  EXACT mode adds the taps in the oracle's order: 0 differences;
    FMA mode: <= 1 LSB and the same bits as the LDS-row kernel."""
    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 77)
    want = oracle_mod.resize(img, ow, oh, filt)
    got_e, u = _up(nsc, alg, img, ow, oh, lanczos_mode="exact")
    assert u.kernel_variant == "resize_down_stream", u.kernel_variant
    assert np.array_equal(got_e, want), (alg, dims, u.kernel_variant, _maxdiff(got_e, want))
    got_f, uf = _up(nsc, alg, img, ow, oh)
    ref_f, ur = _up(nsc, alg, img, ow, oh, options={"force_rows": 1})
    assert ur.kernel_variant == "resize_rows_lds"
    assert np.array_equal(got_f, ref_f) and _maxdiff(got_f, want) <= 1
    check_fma(oracle_mod, got_f, img, ow, oh, filt, (alg, dims, uf.kernel_variant))


@pytest.mark.parametrize("dims", [((464, 64), (232, 32)), ((700, 90), (233, 30)), ((300, 157), (150, 78))])
def test_resize_down_segment_widths(nsc, oracle_mod, dims):
    """The down-scaling kernel's output columns per wave (option down_seg_width; by default the host takes the width whose
    footprint fills whole columns per lane, e.g. 58 at exactly 1/2): every width gives the oracle's bits."""
    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 78)
    want = oracle_mod.resize(img, ow, oh, 0)
    for sw in (0, 64, 58, 57, 50, 41, 1):
        got, u = _up(nsc, "lanczos3", img, ow, oh, lanczos_mode="exact", options={"down_seg_width": sw})
        assert u.kernel_variant == "resize_down_stream"
        assert np.array_equal(got, want), (dims, sw, _maxdiff(got, want))
    u = nsc.PyWgpuUpscaler("quality", "lanczos3")
    u.initialize(w, h, ow, oh)
    with pytest.raises(Exception):
        u.set_option("down_seg_width", 58)  # before initialize only


@pytest.mark.parametrize("dims", [((464, 128), (232, 64)), ((300, 157), (150, 78)), ((384, 216), (256, 144)), ((256, 200), (200, 150))])
def test_resize_down_opaque_and_mixed_alpha_rows(nsc, oracle_mod, dims):
    """FMA mode of the down-scaling kernel on opaque frames, frames whose alpha starts at some row (inside a window, inside a row
    block) and a single transparent pixel: the bits of the LDS-row kernel, within 1 LSB of the oracle; opaque in, opaque out.
    (Written for a 3-channel path for opaque frames -- three channels and one alpha sum per slot until the first row with real
    alpha -- which was built in round 3 and measured SLOWER, 18.0 -> 23.2 us per 4K -> 1080p frame, 19.9 -> 35.4 with alpha:
    profiles/r03_resize_down_opaque_path_ab.txt; the test stays as the guard for any later attempt.)"""
    (w, h), (ow, oh) = dims
    base = oracle_mod.gen_noise(w, h, 41)
    cases = {"opaque": base.copy(), "alpha_from_row": base.copy(), "one_pixel": base.copy(), "alpha_top_only": base.copy()}
    cases["opaque"][..., 3] = 255
    cases["alpha_from_row"][: h // 2 + 3, :, 3] = 255
    cases["one_pixel"][..., 3] = 255
    cases["one_pixel"][h // 3, w // 2, 3] = 7
    cases["alpha_top_only"][5:, :, 3] = 255
    for name, img in cases.items():
        got, u = _up(nsc, "lanczos3", img, ow, oh)
        assert u.kernel_variant == "resize_down_stream"
        ref, ur = _up(nsc, "lanczos3", img, ow, oh, options={"force_rows": 1})
        assert ur.kernel_variant == "resize_rows_lds"
        assert np.array_equal(got, ref), (name, dims, _maxdiff(got, ref))
        assert _maxdiff(got, oracle_mod.resize(img, ow, oh, 0)) <= 1, name
        check_fma(oracle_mod, got, img, ow, oh, 0, (name, dims, u.kernel_variant))
        if name == "opaque":
            assert (got[..., 3] == 255).all()
        for sw in (64, 40):
            got_w, _ = _up(nsc, "lanczos3", img, ow, oh, options={"down_seg_width": sw})
            assert np.array_equal(got_w, ref), (name, dims, sw)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_resize_down_random_shapes(nsc, oracle_mod, seed):
    """Random down-scaling shapes (ratios 1.02 .. 4.7 per axis, widths around the 64-column segment sizes, heights
    around the row-block sizes) through the device batch entry point, whose frame count changes the rows per block;
    EXACT mode, every frame against the oracle."""
    import torch
    rng = np.random.default_rng(900 + seed)
    for case in range(14):
        ow = int(rng.choice([rng.integers(1, 20), rng.integers(60, 70), rng.integers(125, 135), rng.integers(190, 260)]))
        oh = int(rng.choice([rng.integers(1, 12), rng.integers(14, 20), rng.integers(30, 36), rng.integers(60, 140)]))
        w = min(int(ow * rng.uniform(1.0, 4.7)) + int(rng.integers(0, 3)), 1200)
        h = int(oh * rng.uniform(1.02, 4.7)) + 1
        n = int(rng.choice([1, 2, 5]))
        if (w * h) % 4 or (ow * oh) % 4:  # batched device frames must be multiples of 16 bytes
            n = 1
        alg, filt = [("lanczos3", 0), ("bicubic", 1), ("triangle", 2)][case % 3]
        frames = np.stack([oracle_mod.gen_noise(w, h, 1000 * seed + 10 * case + k) for k in range(n)])
        u = nsc.PyWgpuUpscaler("quality", alg, lanczos_mode="exact")
        try:
            u.initialize(w, h, ow, oh)
        except RuntimeError as e:  # windows beyond 32 taps are refused by every resize kernel
            assert "exceeds 32 taps" in str(e), (w, h, ow, oh, str(e))
            continue
        d_in = put(frames)
        d_out = guarded.zeros((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
        u.upscale_device(d_in.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = fetch(d_out)
        for k in range(n):
            want = oracle_mod.resize(frames[k], ow, oh, filt)
            assert np.array_equal(got[k], want), ((w, h), (ow, oh), n, k, alg, u.kernel_variant, _maxdiff(got[k], want))


def test_resize_down_4k_to_1080p_batch(nsc, oracle_mod):
    """The capture-resize case at full size, 3 frames through the device entry point; frame 0 against the oracle."""
    import torch
    w, h, ow, oh = 3840, 2160, 1920, 1080
    frames = np.stack([oracle_mod.gen_noise(w, h, 300 + k) for k in range(3)])
    u = nsc.PyWgpuUpscaler("quality", "lanczos3")
    u.initialize(w, h, ow, oh)
    assert u.kernel_variant == "resize_down_stream"
    d_in = put(frames)
    d_out = guarded.zeros((3, oh, ow, 4), dtype=torch.uint8, device="cuda")
    u.upscale_device(d_in.data_ptr(), d_out.data_ptr(), 3, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = fetch(d_out)
    assert _maxdiff(got[0], oracle_mod.resize(frames[0], ow, oh, 0)) <= 1
    check_fma(oracle_mod, got[0], frames[0], ow, oh, 0, ("4K -> 1080p", u.kernel_variant))
    r = nsc.PyWgpuUpscaler("quality", "lanczos3")
    r.set_option("force_rows", 1)
    r.initialize(w, h, ow, oh)
    for k in range(3):
        assert np.array_equal(got[k], np.frombuffer(r.upscale(frames[k].tobytes()), np.uint8).reshape(oh, ow, 4)), k


@pytest.mark.parametrize("alg", ["nearest", "bilinear", "lanczos3", "bicubic"])
def test_single_frame_in_row_bands(nsc, oracle_mod, alg):
    """upscale() of one frame through the exact-x2 kernels goes band by band (option single_bands, on by default for outputs of
    8 MB and more): the same bytes as the whole-frame path and the oracle's, for heights that are no multiple of anything, rows
    per wave set by the caller, pinned and pageable buffers."""
    for (w, h) in ((1024, 1027), (1600, 700)):
        img = oracle_mod.gen_noise(w, h, 61)
        ow, oh = 2 * w, 2 * h
        whole, uw = _up(nsc, alg, img, ow, oh, options={"single_bands": 0})
        if alg == "nearest":
            assert np.array_equal(whole, oracle_mod.nearest(img, ow, oh))
        elif alg == "bilinear":
            assert np.array_equal(whole, oracle_mod.bilinear(img, ow, oh))
        for th in (0, 7, 24, 40):
            opts = {"single_bands": 1}
            if th and alg in ("lanczos3", "bicubic"):
                opts["rows_per_wave"] = th
            got, u = _up(nsc, alg, img, ow, oh, options=opts)
            assert u.kernel_variant == uw.kernel_variant
            assert np.array_equal(got, whole), (alg, w, h, th, _maxdiff(got, whole))
        u = nsc.PyWgpuUpscaler("quality", alg)
        u.initialize(w, h, ow, oh)
        src, dst = bytearray(img.tobytes()), bytearray(u.output_size)
        with nsc.PinnedBuffer(src), nsc.PinnedBuffer(dst):
            u.upscale_into(src, dst)
        assert np.array_equal(np.frombuffer(dst, np.uint8).reshape(oh, ow, 4), whole), (alg, "pinned")
    with pytest.raises(Exception):
        nsc.PyWgpuUpscaler("quality", alg).set_option("single_bands", 2)


def test_output_piece_plans_give_the_same_bytes(nsc, oracle_mod):
    """A pageable output frame comes back in pieces (options single_out_plan for upscale(), batch_out_chunks for upscale_batch and
    the stream ring): every plan returns the same bytes, on a frame whose size is no multiple of anything and on a tiny one."""
    for (w, h) in ((333, 217), (5, 3), (1920, 1080)):
        img = oracle_mod.gen_noise(w, h, 5)
        want = oracle_mod.nearest(img, 2 * w, 2 * h)
        frames = [img.tobytes()] * 5
        for plan in (0, 1, 2, 3):
            u = nsc.PyWgpuUpscaler("quality", "nearest")
            u.set_option("single_out_plan", plan)
            u.initialize(w, h, 2 * w, 2 * h)
            got = np.frombuffer(u.upscale(img.tobytes()), np.uint8).reshape(2 * h, 2 * w, 4)
            assert np.array_equal(got, want), (w, h, plan)
        for chunks in (1, 2, 3, 8):
            u = nsc.PyWgpuUpscaler("quality", "nearest")
            u.set_option("batch_out_chunks", chunks)
            u.initialize(w, h, 2 * w, 2 * h)
            for out in u.upscale_batch(frames):
                assert np.array_equal(np.frombuffer(out, np.uint8).reshape(2 * h, 2 * w, 4), want), (w, h, chunks)
    u = nsc.PyWgpuUpscaler("quality", "nearest")
    with pytest.raises(Exception):
        u.set_option("batch_out_chunks", 9)
    with pytest.raises(Exception):
        u.set_option("single_out_plan", 4)


def test_c_program_through_the_boundary(nsc, tmp_path):
    """A plain C caller (tests/c_abi/abi_upscale.c) upscales and interpolates through libnuscaler_hip.so."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(nsc._capi.LIB_PATH)
    exe = str(tmp_path / "abi_upscale")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(root, "include"),
           os.path.join(root, "tests", "c_abi", "abi_upscale.c"), "-o", exe, "-L", lib_dir, "-lnuscaler_hip",
           "-Wl,-rpath," + lib_dir]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "abi_upscale ok" in run.stdout, run.stdout + run.stderr


def test_benchmark_api_runs(nsc):
    """The reference's own benchmark entry points over the host path (benchmark.rs:70-272)."""
    r = nsc.py_benchmark_upscaler("wgpu", "ultra", 256, 256, 2.0, 5)
    assert (r.upscaler_name, r.technology, r.quality) == ("WgpuBilinearUpscaler", "Wgpu", "Ultra")
    assert (r.output_width, r.output_height, r.frames_processed) == (512, 512, 5)
    assert r.avg_frame_time_ms > 0 and abs(r.fps - 1000.0 / r.avg_frame_time_ms) < 1e-6 * r.fps
    assert r.total_duration_ms >= r.avg_frame_time_ms * 5 * 0.99
    r2 = nsc.py_benchmark_upscaler("no-such-tech", "no-such-quality", 100, 60, 1.5, 2)
    assert (r2.upscaler_name, r2.technology, r2.quality, r2.output_width, r2.output_height) == \
        ("WgpuNearestUpscaler", "Fallback", "Quality", 150, 90)
    rs = nsc.py_run_comparison_benchmark(64, 64, 2.0, 2)
    assert len(rs) == 16 and {x.technology for x in rs} == {"FSR", "DLSS", "Wgpu", "Fallback"}
    assert all(x.upscaler_name == ("WgpuBilinearUpscaler" if x.technology == "Wgpu" else "WgpuNearestUpscaler") for x in rs)


def test_more_frames_than_one_grid_axis_holds(nsc, oracle_mod):
    """66 000 frames in one device call: the launchers split the batch at 65 535 frames per grid axis; frames on
    both sides of the split (and the second input of the fused blend) must line up."""
    import torch
    n, w, h = 66000, 16, 16
    rng = np.random.default_rng(5)
    frames = put(rng.integers(0, 256, (n + 1, h, w, 4), dtype=np.uint8))
    out = guarded.empty((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    probe = [0, 1, 65534, 65535, 65536, n - 1]
    for alg in ("nearest", "bilinear", "lanczos3"):
        u = nsc.PyWgpuUpscaler("quality", alg, lanczos_mode="exact")
        u.initialize(w, h, 2 * w, 2 * h)
        u.upscale_device(frames.data_ptr(), out.data_ptr(), n, s)
        torch.cuda.synchronize()
        for k in probe:
            want = np.frombuffer(u.upscale(fetch(frames[k]).tobytes()), np.uint8).reshape(2 * h, 2 * w, 4)
            assert np.array_equal(fetch(out[k]), want), (alg, k)
    # fused blend of (frame k, frame k+1) + upscale: the second input must advance with the chunk
    u = nsc.PyWgpuUpscaler("quality", "lanczos3")
    u.initialize(w, h, 2 * w, 2 * h)
    fb = w * h * 4
    u.upscale_blend_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, 0.5, out.data_ptr(), n, s)
    torch.cuda.synchronize()
    for k in probe:
        a, b = fetch(frames[k]), fetch(frames[k + 1])
        mid = oracle_mod.warp_blend(a, b, None, 0.5)
        want = np.frombuffer(u.upscale(mid.tobytes()), np.uint8).reshape(2 * h, 2 * w, 4)
        assert np.array_equal(fetch(out[k]), want), ("fused", k)
    it = nsc.WgpuFrameInterpolator()
    mid_all = guarded.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    it.interpolate_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, 0, w, h, 0.5, mid_all.data_ptr(), n, s)
    torch.cuda.synchronize()
    for k in probe:
        want = oracle_mod.warp_blend(fetch(frames[k]), fetch(frames[k + 1]), None, 0.5)
        assert np.array_equal(fetch(mid_all[k]), want), ("interp", k)


def test_reinitialise_and_destroy_do_not_leak_device_memory(nsc, oracle_mod):
    """Re-initialising with new dimensions frees tables and the three pipeline slots (upscale/mod.rs:883-889 is a
    full re-init too); once the handles are gone the device's free memory is where it was after the same cycle
    had run once before (the first cycle also pays the runtime's one-off code-object and pool allocations)."""
    import gc
    import torch
    probe = nsc.create_advanced_upscaler("quality")

    def cycle(seed):
        rng = np.random.default_rng(seed)
        for alg in ("nearest", "bilinear", "lanczos3", "bicubic", "fsr1"):
            u = nsc.PyWgpuUpscaler("quality", alg)
            for _ in range(6):
                w, h = int(rng.integers(16, 400)), int(rng.integers(16, 300))
                f = float(rng.choice([1.5, 2.0, 3.0, 4.0]))
                ow, oh = int(w * f), int(h * f)
                u.initialize(w, h, ow, oh)
                img = oracle_mod.gen_noise(w, h, 7)
                assert len(u.upscale(img.tobytes())) == ow * oh * 4
                assert len(u.upscale_batch([img.tobytes()] * 4)) == 4
            del u
        it = nsc.WgpuFrameInterpolator()
        for (w, h) in ((64, 64), (640, 360), (1920, 1080), (100, 30)):
            a = oracle_mod.gen_noise(w, h, 8)
            it.interpolate_py(a.tobytes(), a.tobytes(), w, h, flow=np.zeros((h, w, 2), np.float32))
        del it
        gc.collect()
        torch.cuda.synchronize()
        return probe.get_vram_stats().free_mb

    free1 = cycle(9)
    free2 = cycle(9)
    free3 = cycle(10)
    assert abs(free2 - free1) < 32.0 and abs(free3 - free1) < 32.0, (free1, free2, free3)


def test_8k_output_frames(nsc, oracle_mod):
    """4K -> 8K (132 MB per output frame): nearest / bilinear bit-exact against the oracle, Lanczos-3 within 1 LSB
    on a tile-sized sample plus full-frame properties (constant in -> constant out, alpha stays opaque)."""
    w, h = 3840, 2160
    img = oracle_mod.gen_gradient(w, h, 3)
    for alg, ref in (("nearest", oracle_mod.nearest), ("bilinear", oracle_mod.bilinear)):
        got, u = _up(nsc, alg, img, 2 * w, 2 * h)
        assert np.array_equal(got, ref(img, 2 * w, 2 * h, threads=0)), alg
    got, u = _up(nsc, "lanczos3", img, 2 * w, 2 * h)
    assert u.kernel_variant == "lanczos3_x2_regwin"
    want = oracle_mod.lanczos3(img, 2 * w, 2 * h, threads=0)
    assert _maxdiff(got, want) <= 1 and (got != want).mean() < 1e-3
    assert (got[..., 3] == 255).all()
    flat = np.full((h, w, 4), 93, np.uint8)
    got, _ = _up(nsc, "lanczos3", flat, 2 * w, 2 * h)
    assert (got == 93).all()


@pytest.mark.gpu
def test_lanczos_x2_edge_pass_beside_the_main_kernel(nsc, oracle_mod):
    """Batches of >= 8 frames fork the edge-column pass onto the upscaler's second stream (option edge_stream, default 1); the
    main kernel leaves the 8 edge columns per side alone.  Same bytes as with the pass on the caller's stream, every frame's
    edge AND interior columns against the oracle (EXACT mode: 0 differences), plain launch and one-launch step, ragged width."""
    import torch

    w, h, n = 484, 40, 9
    dev = torch.device("cuda:0")
    frames_np = np.stack([oracle_mod.gen_noise(w, h, 800 + k) for k in range(n + 1)])
    frames = put(frames_np)
    s = torch.cuda.current_stream().cuda_stream
    fb = w * h * 4
    outs = {}
    for beside in (1, 0):
        u = nsc.PyWgpuUpscaler("quality", "lanczos3", lanczos_mode="exact")
        u.set_option("edge_stream", beside)
        u.initialize(w, h, 2 * w, 2 * h)
        plain = guarded.zeros((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device=dev)
        u.upscale_device(frames.data_ptr(), plain.data_ptr(), n, s)
        mid = guarded.zeros((n, h, w, 4), dtype=torch.uint8, device=dev)
        up_real, up_mid = guarded.zeros_like(plain), guarded.zeros_like(plain)
        u.upscale_unit_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, 0.5, mid.data_ptr(), up_real.data_ptr(), up_mid.data_ptr(), n, s)
        torch.cuda.synchronize()
        outs[beside] = (plain, up_real, up_mid, mid)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    plain, up_real, up_mid, mid = outs[1]
    assert torch.equal(plain, up_real)
    for k in (0, n - 1):
        want = oracle_mod.lanczos3(frames_np[k], 2 * w, 2 * h)
        got = fetch(plain[k])
        assert np.array_equal(got[:, :8], want[:, :8]) and np.array_equal(got[:, -8:], want[:, -8:]), "edge columns"
        assert np.array_equal(got, want)
        m = oracle_mod.warp_blend(frames_np[k], frames_np[k + 1], None, 0.5)
        assert np.array_equal(fetch(mid[k]), m)
        assert np.array_equal(fetch(up_mid[k]), oracle_mod.lanczos3(m, 2 * w, 2 * h))


@pytest.mark.gpu
def test_probe_device_kinds_move_the_bytes_they_claim(nsc):
    """nus_probe_device (bench.py's box calibration): the copies copy, the 1 R : 4 W stream writes each 16-byte piece four times
    where its header says, the write-only stream fills its range, bad arguments are refused; nothing writes outside its range."""
    import torch

    L = nsc._capi.lib()
    dev = torch.device("cuda:0")
    n = (1 << 20) + 4096 + 48  # not a multiple of the 16-KiB chunk of the stream kernels
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev)
    guard = 4096
    for kind in (0, 1):
        dst = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=dev)
        assert L.nus_probe_device(kind, src.data_ptr(), dst.data_ptr(), n, 0, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst[:n], src) and bool((dst[n:] == 0xA5).all()), kind
    dst = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=dev)
    assert L.nus_probe_device(2, None, dst.data_ptr(), n, 0, None) == 0
    torch.cuda.synchronize()
    w = dst[:n].view(torch.int32).reshape(-1, 4)
    assert torch.equal(w[:, 0], torch.arange(n // 16, dtype=torch.int32, device=dev)) and bool((w[:, 1:] == torch.tensor([1, 2, 3], dtype=torch.int32, device=dev)).all())
    assert bool((dst[n:] == 0xA5).all())
    sink = guarded.zeros(16, dtype=torch.uint8, device=dev)
    assert L.nus_probe_device(3, src.data_ptr(), sink.data_ptr(), n, 0, None) == 0  # read-only: nothing to compare, must not fault
    m = 64 * 1024  # whole waves: 4096 pieces of 16 bytes
    dst = torch.full((4 * m + guard,), 0xA5, dtype=torch.uint8, device=dev)
    assert L.nus_probe_device(4, src.data_ptr(), dst.data_ptr(), m, 0, None) == 0
    torch.cuda.synchronize()
    pieces = src[:m].view(torch.int32).reshape(-1, 64, 4)          # [wave][lane][dword]
    got = dst[:4 * m].view(torch.int32).reshape(-1, 4, 64, 4)      # [wave][copy j][lane][dword]
    for j in range(4):
        assert torch.equal(got[:, j], pieces), j
    assert bool((dst[4 * m:] == 0xA5).all())
    scratch = guarded.zeros(2048 * 256, dtype=torch.float32, device=dev)
    assert L.nus_probe_device(5, None, scratch.data_ptr(), 0, 100, None) == 0
    torch.cuda.synchronize()
    assert float(scratch.abs().max()) == 0.0  # the FMA chains never write
    for bad in ((9, src.data_ptr(), dst.data_ptr(), 16, 0), (1, 0, dst.data_ptr(), 16, 0), (1, src.data_ptr() + 4, dst.data_ptr(), 16, 0),
                (1, src.data_ptr(), dst.data_ptr(), 20, 0), (5, 0, scratch.data_ptr(), 0, 0)):
        assert L.nus_probe_device(bad[0], bad[1] or None, bad[2], bad[3], bad[4], None) != 0


@pytest.mark.parametrize("dims", [((3840, 2160), (7680, 4320)), ((16384, 32), (32768, 64)), ((32, 16384), (64, 32768)), ((8192, 8), (8192 * 3 // 2, 12))])
def test_large_and_extreme_aspect_frames(nsc, oracle_mod, dims):
    """Sizes at the edge of what the reference's own path can hold (its textures stop at 8192 - 16384 a side): 4K -> 8K, a frame 16 384
    pixels wide and 32 tall, one 32 wide and 16 384 tall, an 8192-wide frame at x3/2 -- every filter against the oracle (strip and row-block
    arithmetic, 32-bit offsets inside a frame), outputs between guard bands."""
    import torch

    (w, h), (ow, oh) = dims
    img = oracle_mod.gen_noise(w, h, 321)
    d_in = put(img[None])
    for alg, want, tol in (("nearest", oracle_mod.nearest(img, ow, oh), 0), ("bilinear", oracle_mod.bilinear(img, ow, oh, threads=0), 0),
                           ("lanczos3", oracle_mod.lanczos3(img, ow, oh, threads=0), 1)):
        u = nsc.PyWgpuUpscaler("quality", alg)
        u.initialize(w, h, ow, oh)
        d_out = guarded.empty((1, oh, ow, 4), dtype=torch.uint8, device="cuda")
        u.upscale_device(d_in.data_ptr(), d_out.data_ptr(), 1)
        got = fetch(d_out)[0]
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        assert d.max() <= tol and (tol == 0 or (d > 0).mean() < 1e-3), (alg, u.kernel_variant, int(d.max()), float((d > 0).mean()))
        guarded.assert_intact()
        del d_out
