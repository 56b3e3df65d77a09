"""Frame content of the scene-cut tests: what the detector must and must not call a cut.  numpy only."""
import numpy as np

from nu_scaler_amd.synthetic import gradient_frame, noise_frame


def sine_pattern(w, h, shift=0.0):
    """The textured pattern of the block-matching tests (tests/test_gpu_blockmatch.py: _gradient)."""
    x = np.arange(w, dtype=np.float64)[None, :] - shift
    y = np.arange(h, dtype=np.float64)[:, None]
    v = 127.5 + 45 * np.sin(x / 3.0) * np.cos(y / 4.0) + 50 * np.sin((x + 2 * y) / 23.0) + 25 * np.sin(x / 9.0 + y / 11.0)
    img = np.empty((h, w, 4), np.uint8)
    img[..., 0] = np.clip(v, 0, 255)
    img[..., 1] = np.clip(255 - v, 0, 255)
    img[..., 2] = np.clip(v * 0.5 + 40, 0, 255)
    img[..., 3] = 255
    return img


def brighter(img, step):
    out = img.copy()
    out[..., :3] = np.clip(img[..., :3].astype(np.int64) + step, 0, 255)
    return out


def decision_cases(w, h):
    """[(name, a, b, is a cut, (MAD lo, hi), (histogram permille lo, hi))].  The ranges bracket the figures the contract quotes
    for 320 x 180 (include/nuscaler_hip.h) by a quarter of the figure or more; every case is far from both
    default thresholds (20, 400 permille) on the side that decides it."""
    sine, grad, noise = sine_pattern(w, h), gradient_frame(w, h), noise_frame(w, h)
    black = np.zeros((h, w, 4), np.uint8)
    black[..., 3] = 255
    third = sine.copy()
    third[..., :3] //= 3
    return [
        ("gradient pan 1 px", grad, gradient_frame(w, h, 1), False, (0.5, 1.5), (0, 5)),
        ("gradient pan 24 px", grad, gradient_frame(w, h, 24), False, (14, 25), (0, 5)),
        ("noise shifted 5 px", noise, np.roll(noise, 5, axis=1), False, (75, 95), (0, 5)),
        ("sine pattern shifted 6 px", sine, sine_pattern(w, h, 6.0), False, (21, 35), (0, 30)),
        ("sine pattern + 8 brightness", sine, brighter(sine, 8), False, (6, 10), (150, 340)),
        ("sine pattern -> gradient", sine, grad, True, (50, 80), (560, 860)),
        ("sine pattern -> a third of itself", sine, third, True, (60, 100), (800, 1000)),
        ("gradient -> black", grad, black, True, (95, 160), (800, 1000)),
    ]
