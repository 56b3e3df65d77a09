"""Yardstick of the YUV 4:2:0 kernels (nus_yuv420_to_rgba8* / nus_rgba8_to_yuv420* of include/nuscaler_hip.h, "YUV 4:2:0 frames";
BUILD-DEFINED): the header's integer contract restated in numpy int64 for all 16 (matrix, range, siting, filter) forms and both
directions, and a float64 witness of the same taps with the real-valued coefficients, one floor(x + 0.5) and one clamp.  The GPU
tests ask for the restatement's bytes; tests/test_yuv_contract.py holds the restatement within 1 LSB of the witness.

An I420 frame of w x h: Y plane w*h bytes, then U and V planes of cw*ch bytes each, cw = (w+1)//2, ch = (h+1)//2, rows tight."""
import numpy as np

BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
CENTER, LEFT = 0, 1
NEAREST, BILINEAR = 0, 1
S, H = 14, 1 << 13

FORMS = [(m, r, s, f) for m in (BT601, BT709) for r in (LIMITED, FULL) for s in (CENTER, LEFT) for f in (NEAREST, BILINEAR)]


def frame_bytes(w, h):
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def Q(x):
    return int(np.floor(np.float64(x) * 16384.0 + 0.5))


def _k(matrix):
    kr, kb = ((0.299, 0.114), (0.2126, 0.0722))[matrix]
    return kr, 1.0 - kr - kb, kb


def _range(rng):
    return ((219.0, 224.0, 16), (255.0, 255.0, 0))[rng]


def real_coefficients(matrix, rng):
    """(to_yuv 3x3 rows Y, U, V; to_rgb (cy, rv, bu, gu, gv); Yo) as real numbers."""
    kr, kg, kb = _k(matrix)
    ys, cs, yo = _range(rng)
    yc = [kr * ys / 255.0, kg * ys / 255.0, kb * ys / 255.0]
    uc = [-kr / (2.0 * (1.0 - kb)) * cs / 255.0, -kg / (2.0 * (1.0 - kb)) * cs / 255.0, (1.0 - kb) / (2.0 * (1.0 - kb)) * cs / 255.0]
    vc = [(1.0 - kr) / (2.0 * (1.0 - kr)) * cs / 255.0, -kg / (2.0 * (1.0 - kr)) * cs / 255.0, -kb / (2.0 * (1.0 - kr)) * cs / 255.0]
    rgb = [255.0 / ys, 2.0 * (1.0 - kr) * 255.0 / cs, 2.0 * (1.0 - kb) * 255.0 / cs, -2.0 * kb * (1.0 - kb) / kg * 255.0 / cs,
           -2.0 * kr * (1.0 - kr) / kg * 255.0 / cs]
    return [yc, uc, vc], rgb, yo


def coefficients(matrix, rng):
    """(to_yuv[9], to_rgb[5]) in Q14: what nus_yuv_coefficients returns."""
    m, rgb, _ = real_coefficients(matrix, rng)
    return [Q(c) for row in m for c in row], [Q(c) for c in rgb]


def split(yuv, w, h):
    """(Y[h, w], U[ch, cw], V[ch, cw]) views of one I420 frame."""
    yuv = np.frombuffer(yuv, np.uint8) if not isinstance(yuv, np.ndarray) else yuv.reshape(-1)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert yuv.size == frame_bytes(w, h)
    return (yuv[:w * h].reshape(h, w), yuv[w * h:w * h + cw * ch].reshape(ch, cw), yuv[w * h + cw * ch:].reshape(ch, cw))


def _clampi(a, n):
    return np.clip(a, 0, n - 1)


def _chroma_sums(rgb, siting):
    """Integer-weighted tap sums per chroma cell [ch, cw, 3] (int64) and log2 of the weight total."""
    h, w, _ = rgb.shape
    cw, ch = (w + 1) // 2, (h + 1) // 2
    p = rgb.astype(np.int64)
    ys = [_clampi(2 * np.arange(ch) + j, h) for j in (0, 1)]
    if siting == CENTER:
        taps, lg = [(0, 1), (1, 1)], 2
    else:
        taps, lg = [(-1, 1), (0, 2), (1, 1)], 3
    acc = np.zeros((ch, cw, 3), np.int64)
    for yy in ys:
        for dx, wt in taps:
            xs = _clampi(2 * np.arange(cw) + dx, w)
            acc += wt * p[yy][:, xs]
    return acc, lg


def _dot3(a, c):
    """a[..., 3] . c[3], spelled out (numpy's integer matmul has no fast path)."""
    return a[..., 0] * c[0] + a[..., 1] * c[1] + a[..., 2] * c[2]


def to_yuv(rgb, matrix, rng, siting, real=False, luma=True):
    """rgb [h, w, 3] uint8 -> the I420 frame (uint8 vector).  real: the float64 witness instead of the integer contract.
    luma=False: the U and V planes alone (the exhaustive chroma test has no use for four luma bytes per cell)."""
    h, w, _ = rgb.shape
    m, _, yo = real_coefficients(matrix, rng)
    sums, lg = _chroma_sums(rgb, siting)
    p = rgb.astype(np.int64) if luma else np.zeros((1, 1, 3), np.int64)
    if real:
        mm = np.array(m, np.float64)
        y = np.floor(_dot3(p.astype(np.float64), mm[0]) + yo + 0.5)
        u = np.floor(_dot3(sums.astype(np.float64), mm[1]) / (1 << lg) + 128.0 + 0.5)
        v = np.floor(_dot3(sums.astype(np.float64), mm[2]) / (1 << lg) + 128.0 + 0.5)
    else:
        c = np.array(coefficients(matrix, rng)[0], np.int64).reshape(3, 3)
        y = ((_dot3(p, c[0]) + H) >> S) + yo
        u = ((_dot3(sums, c[1]) + (H << lg)) >> (S + lg)) + 128
        v = ((_dot3(sums, c[2]) + (H << lg)) >> (S + lg)) + 128
    return np.concatenate([np.clip(a, 0, 255).astype(np.uint8).reshape(-1) for a in ((y, u, v) if luma else (u, v))])


def _chroma16(plane, w, h, siting):
    """The bilinear chroma of every luma position [h, w] as an integer sum of weight 16 (int64), 16 * 128 not yet taken off."""
    ch, cw = plane.shape
    c = plane.astype(np.int64)
    y, x = np.arange(h), np.arange(w)
    cy, cx = y >> 1, x >> 1
    ya = np.where(y % 2 == 0, cy - 1, cy)  # weight (1, 3) for even rows, (3, 1) for odd: rows (ya, ya + 1)
    wya = np.where(y % 2 == 0, 1, 3)
    rows = wya[:, None] * c[_clampi(ya, ch)] + (4 - wya)[:, None] * c[_clampi(ya + 1, ch)]  # [h, cw]
    if siting == CENTER:
        xa = np.where(x % 2 == 0, cx - 1, cx)
        wxa = np.where(x % 2 == 0, 1, 3)
    else:
        xa = cx
        wxa = np.where(x % 2 == 0, 4, 2)
    return wxa[None, :] * rows[:, _clampi(xa, cw)] + (4 - wxa)[None, :] * rows[:, _clampi(xa + 1, cw)]


def to_rgb(yuv, w, h, matrix, rng, siting, filt, real=False):
    """One I420 frame -> rgb [h, w, 3] uint8 (alpha is 255 in the library's output)."""
    yp, up, vp = split(yuv, w, h)
    _, rgbc, yo = real_coefficients(matrix, rng)
    yy = yp.astype(np.int64) - yo
    if filt == NEAREST:
        idx = (np.arange(h) >> 1)[:, None], (np.arange(w) >> 1)[None, :]
        u, v, lg = up.astype(np.int64)[idx] - 128, vp.astype(np.int64)[idx] - 128, 0
    else:
        u, v, lg = _chroma16(up, w, h, siting) - 16 * 128, _chroma16(vp, w, h, siting) - 16 * 128, 4
    if real:
        cy, rv, bu, gu, gv = rgbc
        uf, vf = u.astype(np.float64) / (1 << lg), v.astype(np.float64) / (1 << lg)
        r = np.floor(cy * yy + rv * vf + 0.5)
        g = np.floor(cy * yy + gu * uf + gv * vf + 0.5)
        b = np.floor(cy * yy + bu * uf + 0.5)
    else:
        cy, rv, bu, gu, gv = coefficients(matrix, rng)[1]
        base = (cy * yy << lg) + (H << lg)
        r = (base + rv * v) >> (S + lg)
        g = (base + gu * u + gv * v) >> (S + lg)
        b = (base + bu * u) >> (S + lg)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


# ---- the library's RGBA side ------------------------------------------------------------------------------------------------------
ORDER = {0: (0, 1, 2), 1: (2, 1, 0), 2: (0, 1, 2), 3: (2, 1, 0)}  # byte positions of R, G, B in RGBA8 / BGRA8 / RGBX8 / BGRX8


def pack_rgba(rgb, fmt=0):
    """rgb [h, w, 3] -> the library's output pixels [h, w, 4] in nus_pixel_format `fmt`, alpha 255."""
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    for c, pos in enumerate(ORDER[fmt]):
        out[..., pos] = rgb[..., c]
    return out


def unpack_rgba(px, fmt=0):
    """pixels [h, w, 4] in `fmt` -> rgb [h, w, 3] (alpha / X ignored)."""
    return np.stack([px[..., pos] for pos in ORDER[fmt]], axis=-1)


def random_frames(seed, n, w, h):
    """(rgba [n, h, w, 4], yuv [n, frame_bytes]) seeded random bytes."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8), rng.integers(0, 256, (n, frame_bytes(w, h)), dtype=np.uint8)
