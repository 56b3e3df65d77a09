"""numpy-integer restatement of the scene-cut detector's contract (include/nuscaler_hip.h, "Scene-cut detection"): the yardstick
the GPU results must equal bit for bit.  Frames are (h, w, 4) uint8 in the channel order `fmt` names."""
import numpy as np

RGBA, BGRA, RGBX, BGRX = 0, 1, 2, 3  # nus_pixel_format
DEFAULT_MAD, DEFAULT_HIST_PERMILLE = 20, 400


def _rgb(img, fmt):
    """(R, G, B) planes as int64."""
    c = img.astype(np.int64)
    return (c[..., 2], c[..., 1], c[..., 0]) if fmt in (BGRA, BGRX) else (c[..., 0], c[..., 1], c[..., 2])


def luma_hist(img, fmt=RGBA):
    """32 bins of Y >> 3, Y = (77 R + 150 G + 29 B + 128) >> 8."""
    r, g, b = _rgb(img, fmt)
    y = (77 * r + 150 * g + 29 * b + 128) >> 8
    return np.bincount((y >> 3).ravel(), minlength=32).astype(np.int64)


def measures(a, b, fmt=RGBA):
    """-> (sad, hist_l1) as Python integers."""
    sad = int(np.abs(a[..., :3].astype(np.int64) - b[..., :3].astype(np.int64)).sum())
    hist_l1 = int(np.abs(luma_hist(a, fmt) - luma_hist(b, fmt)).sum())
    return sad, hist_l1


def is_cut(sad, hist_l1, w, h, mad_threshold=DEFAULT_MAD, hist_permille=DEFAULT_HIST_PERMILLE):
    """Python integers are unbounded: these are the exact products the device takes in 64 bits."""
    return sad >= mad_threshold * 3 * w * h and hist_l1 * 1000 >= hist_permille * 2 * w * h


def copy_of(img, fmt=RGBA):
    """What the zero-flow interpolation writes for this input at t = 0 / t = 1: RGBA order out, alpha 255 for the X formats."""
    out = img[..., [2, 1, 0, 3]].copy() if fmt in (BGRA, BGRX) else img.copy()
    if fmt in (RGBX, BGRX):
        out[..., 3] = 255
    return out


def apply_cuts(a, b, cut, times, out, fmt=RGBA):
    """a, b: (n, h, w, 4); cut: n flags; out: (n, len(times), h, w, 4), changed in place for the flagged pairs only."""
    for i, c in enumerate(cut):
        if c:
            for k, t in enumerate(times):
                out[i, k] = copy_of(a[i] if np.float32(t) < np.float32(0.5) else b[i], fmt)
    return out


def mad_and_permille(sad, hist_l1, w, h):
    """The two measures in the units of their thresholds (for reading only)."""
    return sad / (3 * w * h), hist_l1 * 1000 / (2 * w * h)
