"""Float64 witness of the optical-flow front end, written from the shaders' definitions (test infrastructure).

Whole-array numpy: every clamped read is an edge-padded array and a slice of it.  Shares no code with `oracle/`; the
C oracle restates the shaders operation by operation in f32, this module states what they compute in float64 -- an
error the two have in common has to be made twice, in two different forms.  Only the stated constants are f32:
the luminance factor 0.33333 (as the shader writes it, not 1/3) and lambda (a f32 uniform).

Images are (h, w, 4) arrays, luminance planes (h, w), flows (h, w, 2) with (dx, dy) per pixel.

`include_centre` / `half_pixel` exist for one purpose: tests/test_flow_witness.py switches them off to show that the
tolerances it asserts tell a wrong stencil from the right one.
"""
import numpy as np

LUM_FACTOR = float(np.float32(0.33333))  # horn_schunck.wgsl: (r + g + b) * 0.33333


def to_float(u8):
    """Rgba8Unorm: u8 / 255."""
    return np.asarray(u8, dtype=np.float64) / 255.0


def _shifted(a, axis, radius):
    """a[i + k] for k = -radius .. radius along `axis`, indices clamped into the array."""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (radius, radius)
    p = np.pad(a, pad, mode="edge")
    n = a.shape[axis]
    sl = [slice(None)] * a.ndim
    out = []
    for k in range(2 * radius + 1):
        sl[axis] = slice(k, k + n)
        out.append(p[tuple(sl)])
    return out


def blur_axis(img, axis):
    m2, m1, c, p1, p2 = _shifted(np.asarray(img, np.float64), axis, 2)
    return (m2 + 4.0 * m1 + 6.0 * c + 4.0 * p1 + p2) / 16.0


def blur(img):
    """Separable 1-4-6-4-1 / 16, clamp to edge: the horizontal pass, then the vertical one."""
    return blur_axis(blur_axis(img, 1), 0)


def downsample(img):
    """2x2 mean; an odd edge reads its last row / column twice.  (h, w) -> ((h+1)//2, (w+1)//2)."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    pad = [(0, h % 2), (0, w % 2)] + [(0, 0)] * (img.ndim - 2)
    p = np.pad(img, pad, mode="edge")
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) * 0.25


def luminance(img):
    img = np.asarray(img, np.float64)
    return (img[..., 0] + img[..., 1] + img[..., 2]) * LUM_FACTOR


def derivatives(l1, l2):
    """(Ix, Iy, It): clamped central differences on frame 1's luminance, It = L2 - L1."""
    xm, _, xp = _shifted(l1, 1, 1)
    ym, _, yp = _shifted(l1, 0, 1)
    return (xp - xm) * 0.5, (yp - ym) * 0.5, l2 - l1


def jacobi_step(ix, iy, it, flow, lam, include_centre=True):
    """One Horn-Schunck Jacobi step: 3x3 mean (with the centre, clamped), then the update."""
    total = np.zeros_like(flow)
    for row in _shifted(flow, 0, 1):
        for cell in _shifted(row, 1, 1):
            total = total + cell
    mean = total / 9.0 if include_centre else (total - flow) / 8.0
    ua, va = mean[..., 0], mean[..., 1]
    common = (ix * ua + iy * va + it) / (lam + ix * ix + iy * iy)
    return np.stack([ua - common * ix, va - common * iy], axis=-1)


def _lambda(lam):
    return float(np.float32(lam))


def horn_schunck(i1, i2, flow_in=None, iterations=1, lam=4e-4, include_centre=True):
    """`iterations` Jacobi steps on two RGBA images, from `flow_in` (zero flow if None)."""
    l1, l2 = luminance(i1), luminance(i2)
    ix, iy, it = derivatives(l1, l2)
    flow = np.zeros(l1.shape + (2,)) if flow_in is None else np.asarray(flow_in, np.float64)
    for _ in range(iterations):
        flow = jacobi_step(ix, iy, it, flow, _lambda(lam), include_centre)
    return flow


def upsample(flow, dw, dh, scale=1.0, half_pixel=True):
    """Bilinear, clamp to edge, pixel centres at half-integers (a linear sampler in texel space); vectors * scale."""
    flow = np.asarray(flow, np.float64)
    sh, sw = flow.shape[:2]

    def axis(n_dst, n_src):
        i = np.arange(n_dst, dtype=np.float64)
        s = (i + 0.5) * n_src / n_dst - 0.5 if half_pixel else i * n_src / n_dst
        i0 = np.floor(s)
        return (np.clip(i0, 0, n_src - 1).astype(np.intp), np.clip(i0 + 1, 0, n_src - 1).astype(np.intp), s - i0)

    x0, x1, fx = axis(dw, sw)
    y0, y1, fy = axis(dh, sh)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = flow[y0][:, x0] * (1.0 - fx) + flow[y0][:, x1] * fx
    bot = flow[y1][:, x0] * (1.0 - fx) + flow[y1][:, x1] * fx
    return (top * (1.0 - fy) + bot * fy) * scale


def pyramid(frame_u8, levels):
    """Luminance of the blurred levels, finest first; stops early once a level is 1x1."""
    cur = to_float(frame_u8)
    out = []
    for level in range(levels):
        b = blur(cur)
        out.append(luminance(b))
        if level + 1 < levels:
            if b.shape[0] == 1 and b.shape[1] == 1:
                break
            cur = downsample(b)
    return out


def estimate(a, b, levels=3, coarse_iters=50, refine_iters=10, lam=4e-4, include_centre=True, half_pixel=True):
    """The estimator: `coarse_iters` steps from zero flow at the coarsest level, then per finer level the flow upsampled
    x2 (vectors doubled) and `refine_iters` more steps."""
    pa, pb = pyramid(a, levels), pyramid(b, levels)
    lam = _lambda(lam)
    top = len(pa) - 1
    ix, iy, it = derivatives(pa[top], pb[top])
    flow = np.zeros(pa[top].shape + (2,))
    for _ in range(coarse_iters):
        flow = jacobi_step(ix, iy, it, flow, lam, include_centre)
    for level in range(top - 1, -1, -1):
        h, w = pa[level].shape
        flow = upsample(flow, w, h, 2.0, half_pixel)
        ix, iy, it = derivatives(pa[level], pb[level])
        for _ in range(refine_iters):
            flow = jacobi_step(ix, iy, it, flow, lam, include_centre)
    return flow
