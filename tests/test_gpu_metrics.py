"""Image-quality metrics on the MI355X (nus_metrics_*, nu_scaler_amd.metrics) against the float64 definition of
tests/_metrics64.py: MSE bit-exact, PSNR within 1e-12 relative, SSIM within 1e-5 absolute; determinism, batching, strides,
stream order, and both command-line tools."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _metrics64 as M64
from conftest import GOLDEN, ROOT, guarded
from nu_scaler_amd.transfer import download, to_device as put, upload

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 5), (11, 11), (17, 13), (320, 240), (1920, 1080), (3840, 2160)]
CONTENTS = ["noise", "gradient", "shifted_gradient", "flat_bright"]


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
    for i in range(n):
        upload(da.data_ptr() + i * sa, np.ascontiguousarray(A[i]), stream)
        upload(db.data_ptr() + i * sb, np.ascontiguousarray(B[i]), stream)
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
        assert abs(got[2] - want_ssim) <= 1e-5, (got[2], want_ssim, got[2] - want_ssim)
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
