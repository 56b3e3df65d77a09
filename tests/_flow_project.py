"""Yardstick of the dense-flow warp's projection rounds (nus_interp_set_flow_project / nus_flow_set_project of
include/nuscaler_hip.h; BUILD-DEFINED): the float64 witness of the rule, the same in numpy float32 with one rounding per operation
(what the GPU is compared with as values), and the quality table DESIGN section 8.1 quotes.  Written for the tests (test
infrastructure, not the product).

The rule.  The flow f lives on frame A's grid; the content that is at output pixel p at time t came from the A-pixel q with
q + t f(q) = p, and its vector is f(q), not f(p).  Per output pixel p = (x, y) of a w x h pair:

    g = f[y][x]
    repeat N times:
        qx = clamp(x - t g.x, 0, w-1);  qy = clamp(y - t g.y, 0, h-1)       (t g.x one product, then one subtraction)
        x0 = floor(qx); x1 = min(x0+1, w-1); fx = qx - x0                   (the same in y)
        top = f[y0][x0] (1-fx) + f[y0][x1] fx;  bot = f[y1][x0] (1-fx) + f[y1][x1] fx
        g   = top (1-fy) + bot fy                                           (per component)

and the warp then uses g in place of f[y][x].  Flows are compared as values (np.array_equal): the kernels may read the border
cell pair (w-2, w-1) with fraction 1 instead of (w-1, w-1) with fraction 0, which can turn a +0 into a -0.  NaN / Inf flows are
out of contract.
"""
import numpy as np

import _bm_bidir as scenes
import _flow_median as M
import _flow_warp64 as W

MAX_PROJECT = 4  # NUS_FLOW_MAX_PROJECT
SETTINGS = ((1, 0), (1, 5), (2, 5))  # (warps, median) of the table
ROUNDS = (0, 1, 2, 3)  # ... and its columns

# PSNR (dB) of the t = 0.5 frame against the rendered true mid-frame, measured with table_row below (float64 witness of the
# estimator, project64, the oracle's warp + blend): MEASURED[(warps, median)][row of W.ROWS] = (rounds 0, 1, 2, 3).
# tests/test_flow_project_yardstick.py holds every cell to these figures minus 0.05 dB; DESIGN section 8.1 quotes the gains.
MEASURED = {
    (1, 0): [
        (31.85, 31.89, 32.13, 31.93),
        (32.15, 33.34, 32.92, 33.23),
        (27.68, 27.71, 27.86, 27.83),
        (34.16, 34.85, 35.14, 35.04),
        (26.44, 26.39, 26.50, 26.46),
        (26.07, 26.67, 26.46, 26.62),
        (23.35, 23.70, 23.57, 23.68),
    ],
    (1, 5): [
        (33.01, 32.85, 33.02, 32.95),
        (33.68, 34.67, 34.28, 34.55),
        (28.20, 28.12, 28.21, 28.20),
        (35.41, 35.72, 35.72, 35.77),
        (26.17, 26.15, 26.20, 26.19),
        (26.84, 27.15, 27.08, 27.14),
        (23.96, 24.18, 24.10, 24.15),
    ],
    (2, 5): [
        (34.43, 34.42, 34.77, 34.63),
        (34.22, 36.26, 35.13, 36.05),
        (29.90, 29.99, 30.21, 30.12),
        (36.16, 37.41, 37.21, 37.47),
        (28.07, 28.07, 28.18, 28.16),
        (28.87, 29.56, 29.28, 29.52),
        (23.89, 24.28, 24.13, 24.24),
    ],
}


def _project(flow, t, rounds, dtype):
    f = np.asarray(flow, dtype)
    if f.ndim != 3 or f.shape[2] != 2 or not 0 <= rounds <= MAX_PROJECT:
        raise ValueError("flow / rounds")
    h, w = f.shape[:2]
    t = dtype(t)
    one, zero = dtype(1), dtype(0)
    x = np.arange(w, dtype=dtype)[None, :]
    y = np.arange(h, dtype=dtype)[:, None]
    g = f.copy()
    for _ in range(rounds):
        qx = np.minimum(np.maximum(x - t * g[..., 0], zero), dtype(w - 1))
        qy = np.minimum(np.maximum(y - t * g[..., 1], zero), dtype(h - 1))
        xf, yf = np.floor(qx), np.floor(qy)
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        fx, fy = (qx - xf)[..., None], (qy - yf)[..., None]
        nfx, nfy = one - fx, one - fy
        top = f[y0, x0] * nfx + f[y0, x1] * fx
        bot = f[y1, x0] * nfx + f[y1, x1] * fx
        g = top * nfy + bot * fy
        assert g.dtype == dtype and g.shape == f.shape
    return g


def project64(flow, t, rounds):
    """The float64 witness: (h, w, 2) flow -> the vector every output pixel is warped with at time t after `rounds` rounds."""
    return _project(flow, t, rounds, np.float64)


def project_f32(flow, t, rounds):
    """The same in float32, one rounding per operation, in the rule's order (t rounded to float32 first): what nus_flow_project
    returns, as values."""
    return _project(flow, t, rounds, np.float32)


def project_loop(flow, t, rounds):
    """project_f32 as a literal per-pixel loop over scalars (the yardstick test compares the two)."""
    f = np.asarray(flow, np.float32)
    h, w = f.shape[:2]
    t = np.float32(t)
    one = np.float32(1)
    out = np.empty_like(f)
    for y in range(h):
        for x in range(w):
            g = f[y, x].copy()
            for _ in range(rounds):
                qx = min(max(np.float32(x) - t * g[0], np.float32(0)), np.float32(w - 1))
                qy = min(max(np.float32(y) - t * g[1], np.float32(0)), np.float32(h - 1))
                x0, y0 = int(np.floor(qx)), int(np.floor(qy))
                x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
                fx, fy = qx - np.float32(x0), qy - np.float32(y0)
                nfx, nfy = one - fx, one - fy
                g = np.empty(2, np.float32)
                for c in range(2):
                    top = f[y0, x0, c] * nfx + f[y0, x1, c] * fx
                    bot = f[y1, x0, c] * nfx + f[y1, x1, c] * fx
                    g[c] = top * nfy + bot * fy
            out[y, x] = g
    return out


# ---- the quality table -------------------------------------------------------------------------------------------------------------
def witness_flow(row, warps, median):
    """The float64 witness estimator's flow of a table scene, rounded to float32 (what the warp reads)."""
    a, b, _ = W.scene(row)
    return M.estimate(a, b, warps=warps, median=median, **W.PARAMS).astype(np.float32)


def table_row(warp_blend, row, settings=SETTINGS, rounds=ROUNDS):
    """-> ({(warps, median, rounds): PSNR (dB) of the t = 0.5 frame against the scene's true mid-frame},
           {(warps, median): the float32 flow});  `warp_blend` is the oracle's."""
    a, b, mid = W.scene(row)
    psnr, flows = {}, {}
    for wn, med in settings:
        flow = flows[wn, med] = witness_flow(row, wn, med)
        for n in rounds:
            g = project64(flow, 0.5, n).astype(np.float32)
            psnr[wn, med, n] = scenes.psnr_rgb(warp_blend(a, b, g, 0.5), mid)
    return psnr, flows


def format_table(rows, settings=SETTINGS, rounds=ROUNDS):
    """Rounds 0 in dB, then the gain of every other round count over it."""
    cols = [(wn, med) for wn, med in settings]
    head = " | ".join(f"warps {wn}, median {med}: rounds 0 (dB) | " + " | ".join(f"rounds {n}" for n in rounds if n) for wn, med in cols)
    out = ["| w×h, pan, square motion (square side) | " + head + " |", "|---|" + "---|" * (len(cols) * len(rounds))]
    for row, psnr in rows:
        w, h, pan, mv, sq = row
        cells = []
        for wn, med in cols:
            cells.append(f"{psnr[wn, med, 0]:.2f}")
            cells += [f"{psnr[wn, med, n] - psnr[wn, med, 0]:+.2f}" for n in rounds if n]
        out.append(f"| {w}×{h}, ({pan[0]},{pan[1]}), ({mv[0]},{mv[1]}) ({sq}) | " + " | ".join(cells) + " |")
    return "\n".join(out)
