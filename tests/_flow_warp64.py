"""Yardstick of the flow estimator's re-linearisation mode (nus_flow_set_warps of include/nuscaler_hip.h): the float64 witness of
the estimator with `warps` rounds per finer level on top of tests/_flow64.py, the same stage restated in numpy float32 operation by
operation (what the GPU primitives are compared with bit for bit), and the quality table DESIGN section 8.1 quotes.  Written for
the tests (test infrastructure, not the product).

A round at a finer level: f0 = (u0, v0) is the level's current flow (round 1: the upsampled coarser flow); L2w is frame B's
luminance sampled bilinearly at (x + u0, y + v0), each coordinate clamped into the plane, pixel centres at integers;
It' = L2w - L1 - Ix u0 - Iy v0; `refine_iters` Jacobi steps from f0 on (Ix, Iy, It').

`nearest` / `linear_terms` exist for one purpose: tests/test_flow_warp_yardstick.py switches them to show that the tolerance it
asserts tells a wrong sampler and a wrong It' from the right ones.
"""
import numpy as np

import _bm_bidir as scenes
import _flow64 as F

MAX_WARPS = 4  # NUS_FLOW_MAX_WARPS

# the rows of the table: w, h, pan, square motion, square side  (the scenes of _bm_bidir.scene, true mid-frame included)
ROWS = [
    (192, 128, (0, 0), (4, 2), 48),
    (192, 128, (-2, 0), (4, 2), 48),
    (192, 128, (0, 0), (6, -2), 48),
    (200, 72, (2, 0), (-4, 2), 32),
    (96, 64, (0, 0), (4, 2), 24),
    (192, 128, (-2, 2), (6, 4), 48),
    (192, 128, (-4, 2), (12, 4), 48),
]
PARAMS = dict(levels=3, coarse_iters=50, refine_iters=10, lam=4e-4)  # the settings of the table

# Distance (max over cells and components, px) of the float32 estimator with warps from the float64 witness, on the scenes of
# ROWS and the 67 x 45 crop the GPU test uses, warps 1 and 2: measured on the CPU with the float32 restatement below (estimate_f32),
# 1.0e-5 .. 1.2e-4 px on flows of up to 35 px, the largest figure 4.4e-4 (192 x 128, pan (-2,2), motion (6,4), warps 2;
# tests/test_flow_warp_yardstick.py prints them all).  The tolerance is four times that largest figure.
F32_MEASURED_MAX = 4.4e-4
F32_TOLERANCE = 4 * F32_MEASURED_MAX


# ---- the lattice of settings tests/test_gpu_flow_warp_lattice.py holds the estimator to ------------------------------------------------
# (w, h, levels, coarse_iters, refine_iters), lambda LATTICE_LAMBDA.  What each row is there for: the level counts 1 .. 4 (rounds
# r >= 2 re-read the flow on one, two and three warped levels in a row; one level warps nothing); refine_iters 1, 5, 6, 7, 10, 13 (the
# launch split of the Jacobi steps, at most 5 a launch, 8 on small tiles, decides which flow buffer a round ends in) and 0 (no round
# at all); coarse_iters 0 (the coarsest level is the memset flow); heights 129 and 257 (2 and 4 row blocks of the streamed
# kernel), widths above 162 (more than three 54-column strips); 333 x 262 and 613 x 517 (the middle and the largest LDS-tile
# class in a batch of a few pairs); sizes below one tile, one lane and one cell.
LATTICE = [
    (65, 33, 2, 50, 7),
    (130, 71, 4, 50, 13),
    (119, 257, 3, 50, 10),
    (173, 70, 3, 0, 10),
    (173, 70, 3, 50, 0),
    (64, 129, 2, 50, 1),
    (64, 129, 1, 50, 10),
    (5, 3, 3, 50, 10),
    (333, 262, 3, 50, 6),
    (613, 517, 2, 50, 5),
    (2, 2, 2, 3, 2),
    (1, 1, 1, 50, 10),
]
LATTICE_LAMBDA = 4e-4
LATTICE_PERIOD = 8  # lattice_frames: frame k is frame k mod 8

# Largest |estimate_f32 - estimate| over LATTICE and warps 1 .. 4, measured on the CPU (tests/test_flow_warp_yardstick.py prints
# every figure): 613 x 517, two levels, 50 + 5 steps, warps 4.  Rounded up; F32_TOLERANCE above stays the bound.
F32_LATTICE_MEASURED_MAX = 6.6e-4


def lattice_frames(w, h, n=2):
    """(n, h, w, 4) RGBA8 frames of a lattice case.  w >= 60 and h >= 30: frame k is the crop [16:16+h, 24:24+w] of
    _bm_bidir.scene(w + 64, h + 64, (-2, 1), (6, 4), 24) with pan and square advanced by k mod 8 steps, so frames 0 and 1 are
    that scene's A and B and the sequence is cyclic with 8 distinct consecutive pairs.  Smaller sizes: noise, two frames."""
    if w >= 60 and h >= 30:
        W_, H_, M, sq, pan, mv = w + 64, h + 64, 64, 24, (-2, 1), (6, 4)
        rng = np.random.default_rng(1)
        bg = scenes.smooth_noise(rng, H_ + 2 * M, W_ + 2 * M)
        fg = scenes.smooth_noise(rng, sq, sq, 1)
        distinct = []
        for k in range(min(n, LATTICE_PERIOD)):
            ox, oy = M + pan[0] * k, M + pan[1] * k
            im = bg[oy:oy + H_, ox:ox + W_].copy()
            x0, y0 = 40 + mv[0] * k, 30 + mv[1] * k
            im[y0:y0 + sq, x0:x0 + sq] = fg
            distinct.append(np.dstack([im, np.full((H_, W_), 255, np.uint8)])[16:16 + h, 24:24 + w])
        return np.ascontiguousarray(np.stack([distinct[k % LATTICE_PERIOD] for k in range(n)]))
    if n != 2:
        raise ValueError("the noise cases are pairs")
    rng = np.random.default_rng(100 * w + h)
    return rng.integers(0, 256, (2, h, w, 4), dtype=np.uint8)


def lattice_id(case):
    w, h, levels, coarse, refine = case
    return f"{w}x{h}-L{levels}-{coarse}+{refine}"


def scene(row):
    w, h, pan, mv, sq = row
    return scenes.scene(w, h, pan, mv, sq)


# ---- float64 witness ------------------------------------------------------------------------------------------------------------
def warp_sample(plane, flow, nearest=False):
    """`plane` (h, w) sampled at (x + u, y + v): bilinear, coordinates clamped into [0, w-1] x [0, h-1], centres at integers."""
    plane = np.asarray(plane, np.float64)
    h, w = plane.shape
    sx = np.clip(np.arange(w, dtype=np.float64)[None, :] + flow[..., 0], 0.0, w - 1.0)
    sy = np.clip(np.arange(h, dtype=np.float64)[:, None] + flow[..., 1], 0.0, h - 1.0)
    if nearest:
        return plane[np.floor(sy + 0.5).astype(np.intp), np.floor(sx + 0.5).astype(np.intp)]
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.astype(np.intp), y0.astype(np.intp)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    top = plane[y0, x0] * (1.0 - fx) + plane[y0, x1] * fx
    bot = plane[y1, x0] * (1.0 - fx) + plane[y1, x1] * fx
    return top * (1.0 - fy) + bot * fy


def coefficients(l1, l2, flow, nearest=False, linear_terms=True):
    """(Ix, Iy, It') of two luminance planes about `flow`."""
    ix, iy, _ = F.derivatives(l1, l2)
    it = warp_sample(l2, flow, nearest) - l1
    if linear_terms:
        it = it - ix * flow[..., 0] - iy * flow[..., 1]
    return ix, iy, it


def estimate(a, b, levels=3, coarse_iters=50, refine_iters=10, lam=4e-4, warps=0, nearest=False, linear_terms=True):
    """_flow64.estimate with `warps` re-linearisation rounds per finer level; warps = 0 is that function, operation for operation."""
    if not 0 <= warps <= MAX_WARPS:
        raise ValueError("warps")
    pa, pb = F.pyramid(a, levels), F.pyramid(b, levels)
    lam = F._lambda(lam)
    top = len(pa) - 1
    ix, iy, it = F.derivatives(pa[top], pb[top])
    flow = np.zeros(pa[top].shape + (2,))
    for _ in range(coarse_iters):
        flow = F.jacobi_step(ix, iy, it, flow, lam)
    for level in range(top - 1, -1, -1):
        h, w = pa[level].shape
        flow = F.upsample(flow, w, h, 2.0)
        if warps == 0 or refine_iters == 0:
            ix, iy, it = F.derivatives(pa[level], pb[level])
            for _ in range(refine_iters):
                flow = F.jacobi_step(ix, iy, it, flow, lam)
            continue
        for _ in range(warps):
            ix, iy, it = coefficients(pa[level], pb[level], flow, nearest, linear_terms)
            for _ in range(refine_iters):
                flow = F.jacobi_step(ix, iy, it, flow, lam)
    return flow


# ---- the stage in float32, one rounding per operation, in the kernels' order ---------------------------------------------------------
_f = np.float32


def luminance_f32(img):
    """(r + g + b) * 0.33333f of an f32 RGBA image, summed left to right."""
    img = np.asarray(img, np.float32)
    return ((img[..., 0] + img[..., 1]) + img[..., 2]) * _f(0.33333)


def coefficients_f32(i1, i2, flow=None):
    """(h, w, 3) float32 (Ix, Iy, It') of two f32 RGBA images about `flow` ((h, w, 2) float32; None: zero flow, It = L2 - L1):
    top = p00*(1-fx) + p10*fx, bot likewise, L2w = top*(1-fy) + bot*fy, It' = ((L2w - L1) - Ix*u0) - Iy*v0."""
    l1, l2 = luminance_f32(i1), luminance_f32(i2)
    h, w = l1.shape
    xs, ys = np.arange(w), np.arange(h)
    xp, xm = np.minimum(xs + 1, w - 1), np.maximum(xs, 1) - 1
    yp, ym = np.minimum(ys + 1, h - 1), np.maximum(ys, 1) - 1
    ix = (l1[:, xp] - l1[:, xm]) * _f(0.5)
    iy = (l1[yp, :] - l1[ym, :]) * _f(0.5)
    if flow is None:
        return np.stack([ix, iy, l2 - l1], axis=-1)
    flow = np.asarray(flow, np.float32)
    u0, v0 = flow[..., 0], flow[..., 1]
    one = _f(1.0)
    sx = np.minimum(np.maximum(xs.astype(np.float32)[None, :] + u0, _f(0.0)), _f(w - 1))
    sy = np.minimum(np.maximum(ys.astype(np.float32)[:, None] + v0, _f(0.0)), _f(h - 1))
    xfl, yfl = np.floor(sx), np.floor(sy)
    fx, fy = sx - xfl, sy - yfl
    x0, y0 = xfl.astype(np.intp), yfl.astype(np.intp)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    top = l2[y0, x0] * (one - fx) + l2[y0, x1] * fx
    bot = l2[y1, x0] * (one - fx) + l2[y1, x1] * fx
    l2w = top * (one - fy) + bot * fy
    it = ((l2w - l1) - ix * u0) - iy * v0
    assert it.dtype == np.float32
    return np.stack([ix, iy, it], axis=-1)


def jacobi_coef_f32(coef, flow, iterations, lam=4e-4):
    """`iterations` Jacobi steps on (h, w, 3) coefficients in float32: the 3 x 3 sum from 0, rows top to bottom and columns left
    to right, / 9, common = ((ix*ua + iy*va) + it) / ((lambda + ix*ix) + iy*iy)."""
    coef = np.asarray(coef, np.float32)
    ix, iy, it = coef[..., 0], coef[..., 1], coef[..., 2]
    den = (_f(lam) + ix * ix) + iy * iy
    h, w = ix.shape
    flow = np.zeros((h, w, 2), np.float32) if flow is None else np.asarray(flow, np.float32)
    ry = [np.clip(np.arange(h) + d, 0, h - 1) for d in (-1, 0, 1)]
    rx = [np.clip(np.arange(w) + d, 0, w - 1) for d in (-1, 0, 1)]
    for _ in range(iterations):
        total = np.zeros_like(flow)
        for yy in ry:
            for xx in rx:
                total = total + flow[yy][:, xx]
        mean = total / _f(9.0)
        ua, va = mean[..., 0], mean[..., 1]
        common = ((ix * ua + iy * va) + it) / den
        flow = np.stack([ua - common * ix, va - common * iy], axis=-1)
    assert flow.dtype == np.float32
    return flow


def estimate_f32(oracle, a, b, levels=3, coarse_iters=50, refine_iters=10, lam=4e-4, warps=1):
    """The estimator with warps >= 1 in float32 on the CPU: the oracle's restatements of the shaders for the pyramid, the coarsest
    level and the upsample, the two functions above for the warped rounds."""
    def pyramid(frame):
        cur, out = oracle.rgba8_to_f32(frame), []
        for level in range(levels):
            cur = oracle.blur(cur)
            out.append(cur)
            if level + 1 < levels:
                if cur.shape[0] == 1 and cur.shape[1] == 1:
                    break
                cur = oracle.downsample(cur)
        return out

    pa, pb = pyramid(a), pyramid(b)
    top = len(pa) - 1
    flow = oracle.horn_schunck(pa[top], pb[top], None, coarse_iters, lam)
    for level in range(top - 1, -1, -1):
        h, w = pa[level].shape[:2]
        flow = oracle.flow_upsample(flow, w, h, 2.0)
        for _ in range(warps if refine_iters else 0):
            flow = jacobi_coef_f32(coefficients_f32(pa[level], pb[level], flow), flow, refine_iters, lam)
    return flow


# ---- the quality table -------------------------------------------------------------------------------------------------------------
def table_row(warp_blend, row, warps=(0, 1, 2)):
    """-> PSNR (dB) of the t = 0.5 frame against the scene's true mid-frame: with zero flow, then with the witness's flow at each
    of `warps`; `warp_blend` is the oracle's."""
    a, b, mid = scene(row)
    out = [scenes.psnr_rgb(warp_blend(a, b, None, 0.5), mid)]
    for wn in warps:
        flow = estimate(a, b, warps=wn, **PARAMS).astype(np.float32)
        out.append(scenes.psnr_rgb(warp_blend(a, b, flow, 0.5), mid))
    return tuple(out)


def format_table(rows):
    out = ["| w×h, pan, square motion (square side) | zero flow | warps 0 | warps 1 | warps 2 |", "|---|---|---|---|---|"]
    for row, (zero, w0, w1, w2) in rows:
        w, h, pan, mv, sq = row
        out.append(f"| {w}×{h}, ({pan[0]},{pan[1]}), ({mv[0]},{mv[1]}) ({sq}) | {zero:.2f} | {w0:.2f} | **{w1:.2f}** | {w2:.2f} |")
    return "\n".join(out)
