"""Yardstick of the flow estimator's median mode (nus_flow_set_median of include/nuscaler_hip.h): the component-wise median in
numpy, the float64 witness of the estimator with the filter behind every Jacobi run on top of tests/_flow_warp64.py, the same in
float32 operation by operation (what the GPU's EXACT mode is compared with as values), and the quality table DESIGN section 8.1
quotes.  Written for the tests (test infrastructure, not the product).

The rule: after every Jacobi run of an estimate -- the coarsest level's `coarse_iters` steps, a finer level's `refine_iters` steps,
with warps each of a finer level's rounds -- the level's flow is replaced by its size x size median, u and v separately, the window
centred on the cell, coordinates clamped into the level.  A run of zero steps is followed by no median.

`pad` / `final_only` exist for one purpose: tests/test_flow_median_yardstick.py switches them to show that the tolerance it
asserts tells zero padding and a filter on the final flow only from the rule.

Flows through the median are compared as values (np.array_equal), not as bit patterns: a sort and a selection network may return
either of -0 and +0.  NaNs are out of contract.
"""
import numpy as np

import _bm_bidir as scenes
import _flow64 as F
import _flow_warp64 as W

SIZES = (3, 5)  # nus_flow_set_median takes these and 0 (off)
MEDIAN_MAX = 5  # NUS_FLOW_MEDIAN_MAX

# Distance (max over cells and components, px) of the float32 estimator with the median from the float64 witness, on the scenes of
# W.ROWS and the 67 x 45 crop, warps 1 and 2, sizes 3 and 5: measured on the CPU with estimate_f32 below, 7.7e-6 .. 7.9e-5 px, the
# largest figure 9.3e-5 (192 x 128, pan (-4,2), motion (12,4), warps 2, 3 x 3; tests/test_flow_median_yardstick.py prints them all
# and holds the recorded figure to the measured maximum).  With warps = 0 the same cases give at most 3.5e-5.  The tolerance is four
# times the largest figure, as W.F32_TOLERANCE is set.  (Without the median the same estimator is up to 4.4e-4 px from its witness: a
# median is non-expansive in the max norm and discards the cells that have drifted furthest.)
F32_MEASURED_MAX = 9.3e-5
F32_TOLERANCE = 4 * F32_MEASURED_MAX


def median_filter(flow, size, pad="edge"):
    """(h, w, 2) -> its component-wise size x size median: edge padding, a sliding window, the middle element of the sorted window."""
    if size not in SIZES:
        raise ValueError("size")
    flow = np.asarray(flow)
    r = size // 2
    p = np.pad(flow, ((r, r), (r, r), (0, 0)), mode=pad)
    win = np.lib.stride_tricks.sliding_window_view(p, (size, size), axis=(0, 1))  # (h, w, 2, size, size)
    win = win.reshape(flow.shape + (size * size,))
    out = np.sort(win, axis=-1)[..., size * size // 2]
    assert out.dtype == flow.dtype and out.shape == flow.shape
    return out


def _filter(median, pad, final_only):
    if median == 0 or final_only:
        return lambda flow: flow
    return lambda flow: median_filter(flow, median, pad)


# ---- float64 witness ------------------------------------------------------------------------------------------------------------
def estimate(a, b, levels=3, coarse_iters=50, refine_iters=10, lam=4e-4, warps=0, median=0, pad="edge", final_only=False):
    """_flow_warp64.estimate with the median behind every Jacobi run; median = 0 is that function, operation for operation."""
    if not 0 <= warps <= W.MAX_WARPS or median not in (0,) + SIZES:
        raise ValueError("warps / median")
    filt = _filter(median, pad, final_only)
    pa, pb = F.pyramid(a, levels), F.pyramid(b, levels)
    lam = F._lambda(lam)
    top = len(pa) - 1
    ix, iy, it = F.derivatives(pa[top], pb[top])
    flow = np.zeros(pa[top].shape + (2,))
    for _ in range(coarse_iters):
        flow = F.jacobi_step(ix, iy, it, flow, lam)
    if coarse_iters:
        flow = filt(flow)
    for level in range(top - 1, -1, -1):
        h, w = pa[level].shape
        flow = F.upsample(flow, w, h, 2.0)
        if refine_iters == 0:
            continue
        if warps == 0:
            ix, iy, it = F.derivatives(pa[level], pb[level])
            for _ in range(refine_iters):
                flow = F.jacobi_step(ix, iy, it, flow, lam)
            flow = filt(flow)
            continue
        for _ in range(warps):
            ix, iy, it = W.coefficients(pa[level], pb[level], flow)
            for _ in range(refine_iters):
                flow = F.jacobi_step(ix, iy, it, flow, lam)
            flow = filt(flow)
    if final_only and median:
        flow = median_filter(flow, median, pad)
    return flow


# ---- the same in float32, one rounding per operation, in the kernels' order ---------------------------------------------------------
def estimate_f32(oracle, a, b, levels=3, coarse_iters=50, refine_iters=10, lam=4e-4, warps=0, median=0):
    """The estimator in float32 on the CPU: the oracle's restatements of the shaders for the pyramid, the coarsest level, the
    upsample and -- warps = 0 -- the finer levels' steps (horn_schunck), _flow_warp64's two functions for the warped rounds, and
    median_filter behind every run of at least one step.  median = 0: oracle.flow_estimate (warps 0) / _flow_warp64.estimate_f32."""
    if not 0 <= warps <= W.MAX_WARPS or median not in (0,) + SIZES:
        raise ValueError("warps / median")
    filt = _filter(median, "edge", False)

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
    if coarse_iters:
        flow = filt(flow)
    for level in range(top - 1, -1, -1):
        h, w = pa[level].shape[:2]
        flow = oracle.flow_upsample(flow, w, h, 2.0)
        if refine_iters == 0:
            continue
        if warps == 0:
            flow = filt(oracle.horn_schunck(pa[level], pb[level], flow, refine_iters, lam))
            continue
        for _ in range(warps):
            flow = filt(W.jacobi_coef_f32(W.coefficients_f32(pa[level], pb[level], flow), flow, refine_iters, lam))
    flow = np.asarray(flow)
    assert flow.dtype == np.float32
    return flow


# ---- the quality table -------------------------------------------------------------------------------------------------------------
TABLE_WARPS = (1, 2)


def table_row(warp_blend, row, warps=TABLE_WARPS, sizes=SIZES):
    """-> {(warps, size): PSNR (dB) of the t = 0.5 frame against the scene's true mid-frame}, size 0 included; the flow is the
    float64 witness's, `warp_blend` the oracle's."""
    a, b, mid = W.scene(row)
    out = {}
    for wn in warps:
        for size in (0,) + tuple(sizes):
            flow = estimate(a, b, warps=wn, median=size, **W.PARAMS).astype(np.float32)
            out[wn, size] = scenes.psnr_rgb(warp_blend(a, b, flow, 0.5), mid)
    return out


def format_table(rows, warps=TABLE_WARPS, sizes=SIZES):
    """Gain in dB over the same estimator without the median."""
    cols = [(wn, s) for wn in warps for s in sizes]
    out = ["| w×h, pan, square motion (square side) | " + " | ".join(f"warps {wn}, {s}×{s}" for wn, s in cols) + " |",
           "|---|" + "---|" * len(cols)]
    for row, psnr in rows:
        w, h, pan, mv, sq = row
        gains = " | ".join(f"{psnr[wn, s] - psnr[wn, 0]:+.2f}" for wn, s in cols)
        out.append(f"| {w}×{h}, ({pan[0]},{pan[1]}), ({mv[0]},{mv[1]}) ({sq}) | {gains} |")
    return "\n".join(out)
