"""Image-quality metrics on the MI355X (nus_metrics_*, nu_scaler_amd.metrics) against the float64 definition of
tests/_metrics64.py: MSE bit-exact, PSNR within 1e-12 relative, SSIM within SSIM_TOL absolute; determinism, batching, strides,
stream order, and both command-line tools.

The SSIM contract is 1e-5 absolute (include/nuscaler_hip.h).  What is asserted is tighter: SSIM_TOL = 5.6e-7, four times the worst
distance between the restatement of the kernel's arithmetic (_metrics64.ssim_kernel_model: f64 window statistics and differences,
f32 ratio) and the definition, measured on the CPU over every class below; the factor covers one ulp of the f32 divide and another
libm.  Worst |model - definition| per class (tests/test_metrics_reference.py asserts them), and in brackets the same for the
all-f32 arithmetic the kernel had before (the MI355X gave the same figures with either kernel, to every digit shown):
    constant pairs (c, c+1 / c-1 / c-2 / c+5), 1015 of 24 x 20       1.25e-7   [1.17e-4, 445 pairs above 1e-5]
    the same with R = c, G = 255 - c, B = 128                        6.5e-8    [7.2e-5, 266 pairs above 1e-5]
    stripes and checkerboards of two levels, 30 x 28 and 139 x 75    1.31e-7   [4.4e-5]
    letterbox / pillarbox bars 16 against 17 around a noise picture  5.7e-10   [4.2e-6]
    tile-edge shapes, independent noise                              8.6e-9    [1.9e-8]
    SHAPES x CONTENTS below (noise, gradients, the 250/251 mix)      1.12e-7   [8.9e-6]
On flat and few-valued frames every window makes the same rounding error, so the mean over the windows keeps it; on noise the
errors average out, which is why noise alone could not hold the kernel to its contract.  The tile-edge shapes are the other kind
of case: at 74 x 42 .. 139 x 75 one wrong, missing or doubled window moves the mean by 1e-4 or more, 200 times the tolerance."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _metrics64 as M64
import _metrics_cases as MC
from conftest import GOLDEN, ROOT, guarded
from nu_scaler_amd.transfer import download, to_device as put, upload

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 5), (11, 11), (17, 13), (320, 240), (1920, 1080), (3840, 2160)]
CONTENTS = ["noise", "gradient", "shifted_gradient", "flat_bright"]
SSIM_TOL = MC.SSIM_TOL


def _pair(kind, w, h, seed=0):
    rng = np.random.default_rng(seed + 7 * w + 13 * h)
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, 4), dtype=np.int32)
        b = np.clip(a + rng.integers(-24, 25, (h, w, 4)), 0, 255)
    elif kind in ("gradient", "shifted_gradient"):
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1),
                      rng.integers(0, 256, (h, w))], axis=-1)
        if kind == "gradient":
            b = np.clip(a + rng.integers(-3, 4, (h, w, 4)), 0, 255)
        else:
            b = np.roll(a, (1, 2), axis=(0, 1))
    elif kind == "flat_bright":
        a = 250 + rng.integers(0, 2, (h, w, 4))
        b = np.clip(251 + rng.integers(-1, 2, (h, w, 4)), 0, 255)
    else:
        raise ValueError(kind)
    return a.astype(np.uint8), b.astype(np.uint8)


def _golden_pair():
    from _png import read_png

    a = read_png(os.path.join(GOLDEN, "ref_test_input.png"))
    rng = np.random.default_rng(5)
    b = np.clip(a.astype(np.int32) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    return a, b


def _device_metrics(nsc, A, B, mse=True, ssim=True, a_stride=None, b_stride=None, stream=0):
    """Metrics of the pairs (A[i], B[i]) through nus_metrics_compare_device; frames at the given strides, gaps poisoned."""
    import torch

    from nu_scaler_amd import metrics

    n, h, w = A.shape[:3]
    fb = h * w * 4
    sa, sb = a_stride or fb, b_stride or fb
    da = torch.full((n * sa,), 0xA5, dtype=torch.uint8, device="cuda")
    db = torch.full((n * sb,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for d, X, sx in ((da, A, sa), (db, B, sb)):
        if sx == fb:  # frames back to back: one copy
            upload(d.data_ptr(), np.ascontiguousarray(X), stream)
        else:
            for i in range(n):
                upload(d.data_ptr() + i * sx, np.ascontiguousarray(X[i]), stream)
    ws_n = metrics.workspace_size(w, h, n, mse=mse, ssim=ssim)
    ws = guarded.empty(ws_n, dtype=torch.uint8, device="cuda")
    out = guarded.empty(n * 3, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    metrics.compare_device(da.data_ptr(), sa, db.data_ptr(), sb, w, h, n, ws.data_ptr(), ws_n, out.data_ptr(), mse=mse, ssim=ssim,
                           stream=stream)
    res = np.empty(n * 3, np.float64)
    download(out.data_ptr(), res.nbytes, res, stream)
    return res.reshape(n, 3)


def _check(got, a, b, ssim=True):
    want_mse = M64.mse(a, b)
    assert got[0] == want_mse, (got[0], want_mse)  # bit-exact
    want_psnr = M64.psnr_of(want_mse)
    if math.isinf(want_psnr):
        assert got[1] == math.inf
    else:
        assert abs(got[1] - want_psnr) <= 1e-12 * abs(want_psnr) + 1e-300, (got[1], want_psnr)
    if ssim:
        want_ssim = M64.ssim(a, b)
        assert abs(got[2] - want_ssim) <= SSIM_TOL, (got[2], want_ssim, got[2] - want_ssim)
    else:
        assert math.isnan(got[2])


def test_device_present(nsc):
    assert nsc.device_count() >= 1


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", CONTENTS)
def test_metrics_against_float64(nsc, shape, kind):
    w, h = shape
    a, b = _pair(kind, w, h)
    ssim = w >= 11 and h >= 11
    got = _device_metrics(nsc, a[None], b[None], ssim=ssim)[0]
    _check(got, a, b, ssim)
    if ssim:  # SSIM alone: the same SSIM bytes, no MSE
        only = _device_metrics(nsc, a[None], b[None], mse=False, ssim=True)[0]
        assert math.isnan(only[0]) and math.isnan(only[1]) and only[2] == got[2]
    # MSE alone equals MSE next to SSIM, bit for bit
    alone = _device_metrics(nsc, a[None], b[None], mse=True, ssim=False)[0]
    assert alone[0] == got[0] and alone[1] == got[1] and math.isnan(alone[2])


def test_golden_image_against_perturbed_copy(nsc):
    a, b = _golden_pair()
    assert a.shape == (240, 320, 4)
    _check(_device_metrics(nsc, a[None], b[None])[0], a, b)


def test_black_against_white_4k_has_no_overflow(nsc):
    a = np.zeros((2160, 3840, 4), np.uint8)
    b = np.full((2160, 3840, 4), 255, np.uint8)
    for ssim in (False, True):
        got = _device_metrics(nsc, a[None], b[None], ssim=ssim)[0]
        assert got[0] == 65025.0 and got[1] == 0.0, got


@pytest.mark.parametrize("shape", [(11, 11), (320, 240), (1920, 1080)])
def test_identical_frames(nsc, shape):
    w, h = shape
    a, _ = _pair("noise", w, h)
    got = _device_metrics(nsc, a[None], a[None])[0]
    assert got[0] == 0.0 and got[1] == math.inf and got[2] == 1.0, got


def _check_batch(got, name, labels=None):
    """Every pair of a _metrics_cases batch: MSE bit-exact, PSNR within 1e-12 relative, SSIM within SSIM_TOL of the definition."""
    A, B = MC.batch(name)
    h, w = A.shape[1:3]
    d = A[..., :3].astype(np.int64) - B[..., :3].astype(np.int64)
    want_mse = (d * d).sum(axis=(1, 2, 3)) / (float(w * h) * 3.0)
    assert np.array_equal(got[:, 0], want_mse), np.flatnonzero(got[:, 0] != want_mse)[:8]
    for i, m in enumerate(want_mse):
        want_psnr = M64.psnr_of(float(m))
        assert got[i, 1] == want_psnr if math.isinf(want_psnr) else abs(got[i, 1] - want_psnr) <= 1e-12 * abs(want_psnr), (i, got[i])
    err = np.abs(got[:, 2] - MC.witness(name))
    bad = np.flatnonzero(~(err <= SSIM_TOL))
    print(f"{name}: worst |ssim - float64| {err.max():.3e} at pair {int(err.argmax())}; {bad.size} of {len(err)} above {SSIM_TOL:.1e},"
          f" {int((err > 1e-5).sum())} above 1e-5")
    assert bad.size == 0, (name, bad.size, float(err.max()),
                           [(labels[i] if labels else int(i), float(got[i, 2]), float(err[i])) for i in bad[np.argsort(-err[bad])][:6]])


@pytest.mark.parametrize("name", ["constant", "constant_rgb"])
def test_constant_pairs(nsc, name):
    """Frames of one level against one level a step away (letterbox black 16 against 17 among them): 1015 pairs of 24 x 20 in one
    call; then with a different level in each channel.  In f32, E[x^2] - mu^2 of such a window is off by up to 1e-3 against
    C2 = 58.5, the same in every window of the frame."""
    A, B = MC.batch(name)
    got = _device_metrics(nsc, A, B)
    _check_batch(got, name, labels=MC.constant_pair_levels())
    only = _device_metrics(nsc, A, B, mse=False, ssim=True)  # SSIM alone: the same SSIM bytes
    assert only[:, 2].tobytes() == got[:, 2].tobytes() and np.isnan(only[:, :2]).all()
    alone = _device_metrics(nsc, A, B, mse=True, ssim=False)  # MSE and PSNR do not depend on SSIM being asked
    assert alone[:, :2].tobytes() == got[:, :2].tobytes() and np.isnan(alone[:, 2]).all()
    same = _device_metrics(nsc, A, A)
    assert np.all(same[:, 0] == 0.0) and np.all(same[:, 1] == math.inf) and np.all(same[:, 2] == 1.0)


@pytest.mark.parametrize("size", MC.PERIODIC_SIZES)
def test_few_valued_periodic_content(nsc, size):
    """Stripes and checkerboards of two levels, period 2 and 3, against themselves a level away, rolled by a pixel and against a
    constant: 90 pairs in one call, one tile at 30 x 28 and six at 139 x 75."""
    name = f"periodic_{size[0]}x{size[1]}"
    A, B = MC.batch(name)
    got = _device_metrics(nsc, A, B)
    _check_batch(got, name, labels=MC.periodic_pairs(*size)[0])
    again = _device_metrics(nsc, A, B)
    assert again.tobytes() == got.tobytes()
    same = _device_metrics(nsc, B, B)
    assert np.all(same[:, 0] == 0.0) and np.all(same[:, 2] == 1.0)


@pytest.mark.parametrize("name", ["letterbox", "pillarbox"])
def test_letterbox_bars_one_level_apart(nsc, name):
    """The same noise picture between bars of 16 in one frame and 17 in the other; windows inside the bars are constant pairs,
    windows across the bar's edge see a flat half and a noisy half."""
    A, B = MC.batch(name)
    _check_batch(_device_metrics(nsc, A, B), name)


@pytest.mark.parametrize("shape", MC.TILE_EDGE_SHAPES)
def test_tile_edge_shapes(nsc, shape):
    """Independent noise at the sizes where the 64 x 32 tiling changes: one tile exactly, one more column and / or row of centres,
    2 x 2 tiles and one more, and frames one window thin.  The middle pair alone and inside a batch of three at strides that are
    not a multiple of 16: the same bytes; identical frames: exactly 1."""
    w, h = shape
    name = f"tile_{w}x{h}"
    A, B = MC.batch(name)
    fb = w * h * 4
    batch = _device_metrics(nsc, A, B, a_stride=fb + 12, b_stride=fb + 12)
    _check_batch(batch, name)
    single = _device_metrics(nsc, A[1:2], B[1:2])
    assert single[0].tobytes() == batch[1].tobytes(), (single[0], batch[1])
    assert _device_metrics(nsc, A, B, a_stride=fb + 12, b_stride=fb + 12).tobytes() == batch.tobytes()
    for ssim_only in (False, True):
        same = _device_metrics(nsc, A, A, mse=not ssim_only, a_stride=fb + 12)
        assert np.all(same[:, 2] == 1.0), same
    alone = _device_metrics(nsc, A, B, ssim=False)
    assert alone[:, :2].tobytes() == batch[:, :2].tobytes()


def test_alpha_is_ignored(nsc):
    a, b = _pair("noise", 200, 150)
    a2, b2 = a.copy(), b.copy()
    a2[..., 3] = 255 - a[..., 3]
    b2[..., 3] = 17
    assert np.array_equal(_device_metrics(nsc, a[None], b[None]), _device_metrics(nsc, a2[None], b2[None]))


@pytest.mark.parametrize("shape", [(200, 150), (75, 43), (11, 11), (64 + 10, 32 + 10), (64 + 11, 32 + 11)])
def test_single_pixel_differences_give_the_exact_sse(nsc, shape):
    """One differing pixel in each corner and at tile borders: the SSE counts each pixel exactly once (no lost or double-counted
    halo or border pixel), with SSIM or without."""
    w, h = shape
    a = np.full((h, w, 4), 100, np.uint8)
    spots = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (5, 5), (w - 6, h - 6), (min(68, w - 1), min(36, h - 1)),
             (min(69, w - 1), min(37, h - 1)), (4, min(37, h - 1)), (min(69, w - 1), 4)}
    for ssim in (False, True):
        for x, y in sorted(spots):
            b = a.copy()
            b[y, x, :3] = (103, 95, 100)  # SSE 9 + 25
            got = _device_metrics(nsc, a[None], b[None], ssim=ssim)[0]
            assert got[0] * 3.0 * w * h == 34.0, (x, y, ssim, got)
        b = a.copy()
        for x, y in spots:
            b[y, x, 1] = 90
        got = _device_metrics(nsc, a[None], b[None], ssim=ssim)[0]
        assert got[0] == M64.mse(a, b), (ssim, got[0] * 3 * w * h, M64.sse(a, b))


@pytest.mark.parametrize("mse,ssim", [(True, False), (True, True), (False, True)])
def test_batch_with_strides_equals_single_calls(nsc, mse, ssim):
    w, h, n = 37, 23, 5  # odd W*H; strides a multiple of 4 bytes but not of 16: misaligned frame bases
    fb = w * h * 4
    pairs = [_pair(k, w, h, seed=i) for i, k in enumerate(["noise", "gradient", "shifted_gradient", "flat_bright", "noise"])]
    A = np.stack([p[0] for p in pairs])
    B = np.stack([p[1] for p in pairs])
    batch = _device_metrics(nsc, A, B, mse=mse, ssim=ssim, a_stride=fb + 12, b_stride=fb + 260)
    for i in range(n):
        single = _device_metrics(nsc, A[i:i + 1], B[i:i + 1], mse=mse, ssim=ssim)[0]
        assert batch[i].tobytes() == single.tobytes(), (i, batch[i], single)
        if mse:
            assert batch[i][0] == M64.mse(A[i], B[i])


def test_runs_are_byte_identical(nsc):
    A = np.stack([_pair("noise", 1920, 1080, seed=s)[0] for s in range(3)])
    B = np.stack([_pair("noise", 1920, 1080, seed=s)[1] for s in range(3)])
    r1 = _device_metrics(nsc, A, B)
    r2 = _device_metrics(nsc, A, B)
    assert r1.tobytes() == r2.tobytes()
    for i in range(3):  # every batch position equals its own single call
        assert _device_metrics(nsc, A[i:i + 1], B[i:i + 1]).tobytes() == r1[i:i + 1].tobytes()


@pytest.mark.parametrize("shape", [(7, 5), (320, 240), (1920, 1080)])
def test_host_entry_point_equals_device_entry_point(nsc, shape):
    from nu_scaler_amd.metrics import ErrorMetrics

    w, h = shape
    a, b = _pair("gradient", w, h)
    ssim = w >= 11 and h >= 11
    dev = _device_metrics(nsc, a[None], b[None], ssim=ssim)[0]
    em = ErrorMetrics.calculate(a, b)
    assert np.array([em.mse(), em.psnr(), em.ssim()]).tobytes() == dev.tobytes()
    em2 = ErrorMetrics.calculate(a, b)  # the kept device buffers give the same bytes again
    assert (em2.mse(), em2.psnr()) == (em.mse(), em.psnr())


def test_host_entry_point_reuses_its_grown_buffers(nsc):
    """nus_metrics_compare on one device with a 16x12 pair, a 48x32 pair (the kept buffers grow) and the 16x12 pair again (they
    are reused, larger than needed): each result against the float64 definition, the third the bytes of the first."""
    from nu_scaler_amd.metrics import ErrorMetrics

    res = []
    for w, h in ((16, 12), (48, 32), (16, 12)):
        a, b = _pair("noise", w, h)
        em = ErrorMetrics.calculate(a, b)
        res.append(np.array([em.mse(), em.psnr(), em.ssim()]))
        _check(res[-1], a, b)
    assert res[2].tobytes() == res[0].tobytes()


def test_scores_gpu_lanczos_on_the_same_stream(nsc, oracle_mod):
    """upscale_device, then compare_device on the same non-null stream with no synchronisation between them: the GPU
    Lanczos-3 x2 (FMA mode, within 1 LSB) against the oracle's output."""
    import torch

    w, h = 320, 240
    img = oracle_mod.gen_noise(w, h, 31)
    want = oracle_mod.lanczos3(img, 2 * w, 2 * h)
    u = nsc.PyWgpuUpscaler("quality", "lanczos3")
    u.initialize(w, h, 2 * w, 2 * h)
    d_in = put(img)
    d_want = put(want)
    d_up = guarded.empty(2 * h, 2 * w, 4, dtype=torch.uint8, device="cuda")
    ws_n = nsc.metrics.workspace_size(2 * w, 2 * h, 1)
    ws = guarded.empty(ws_n, dtype=torch.uint8, device="cuda")
    out = guarded.empty(3, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    u.upscale_device(d_in.data_ptr(), d_up.data_ptr(), 1, s.cuda_stream)
    nsc.metrics.compare_device(d_up.data_ptr(), 4 * w * h * 4, d_want.data_ptr(), 4 * w * h * 4, 2 * w, 2 * h, 1, ws.data_ptr(), ws_n,
                               out.data_ptr(), stream=s.cuda_stream)
    res = np.empty(3, np.float64)
    download(out.data_ptr(), res.nbytes, res, s.cuda_stream)
    up = np.empty((2 * h, 2 * w, 4), np.uint8)
    download(d_up.data_ptr(), up.nbytes, up, s.cuda_stream)
    _check(res, up, want)
    assert res[1] >= 48.0, res


def _write_png(path, img):
    from nu_scaler_amd.imagefile import write_png

    write_png(str(path), img.shape[1], img.shape[0], np.ascontiguousarray(img).tobytes())


def test_both_command_line_tools_print_the_same_line(nsc, tmp_path):
    from nu_scaler_amd.metrics import ErrorMetrics

    cli = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    assert os.path.exists(cli)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for (w, h), kind in (((96, 64), "noise"), ((9, 7), "gradient")):
        a, b = _pair(kind, w, h)
        pa, pb = tmp_path / f"a{w}.png", tmp_path / f"b{w}.png"
        _write_png(pa, a)
        _write_png(pb, b)
        native = subprocess.run([cli, "compare", str(pa), str(pb)], capture_output=True, text=True, timeout=120)
        py = subprocess.run([sys.executable, "-m", "nu_scaler_amd.cli", "compare", str(pa), str(pb)], capture_output=True, text=True,
                            timeout=300, cwd=ROOT, env=env)
        assert native.returncode == 0 and py.returncode == 0, (native.stderr, py.stderr)
        assert native.stdout == py.stdout, (native.stdout, py.stdout)
        assert native.stdout.strip() == ErrorMetrics.calculate(a, b).line()
        if w < 11 or h < 11:
            assert native.stdout.strip().endswith("ssim=nan")
    # different sizes: the reference's error, exit status 1
    _write_png(tmp_path / "c.png", _pair("noise", 95, 64)[0])
    for cmd in ([cli], [sys.executable, "-m", "nu_scaler_amd.cli"]):
        r = subprocess.run(cmd + ["compare", str(tmp_path / "a96.png"), str(tmp_path / "c.png")], capture_output=True, text=True,
                           timeout=300, cwd=ROOT, env=env)
        assert r.returncode == 1 and "Images must have the same dimensions" in r.stderr, (cmd, r.stderr)
