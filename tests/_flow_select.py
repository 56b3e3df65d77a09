"""Yardstick of the select warp (nus_interp_interpolate_select_device of include/nuscaler_hip.h; BUILD-DEFINED): each output pixel
is warped with the forward flow's vector or with the negated backward flow's, whichever makes its two samples agree better.  The
rule restated in numpy float32 with one rounding per operation (what the EXACT kernels are compared with byte for byte), the same
as a literal per-pixel loop, and the quality table DESIGN section 8.1 quotes.  Written for the tests (test infrastructure, not the
product).

The rule.  F is the flow A -> B on A's grid, R the flow B -> A on B's grid, N the projection rounds, nt = 1 - t in float32:

    gF = F projected N rounds at time t          (tests/_flow_project.py)
    gR = -(R projected N rounds at time nt)      (the content at p came from the B-pixel q with q + nt R(q) = p)
    per candidate g:  sa = A sampled at p - t g,  sb = B sampled at p + nt g, both truncated to a count (the oracle's sampling)
    e(g) = |sa0 - sb0| + |sa1 - sb1| + |sa2 - sb2|      (the three colour bytes as stored; alpha does not vote)
    the backward candidate wins iff e(gR) < e(gF); a tie goes forward
    pixel = trunc(nt sa + t sb) of the winner's samples (three roundings)
"""
import numpy as np

import _bm_bidir as scenes
import _flow_median as M
import _flow_project as PJ
import _flow_warp64 as W
from oracle import oracle_np

_f = np.float32

SETTINGS = ((1, 0), (2, 5))  # (warps, median) of the table
ROUNDS = (0, 3)  # ... and its projection rounds
KINDS = ("forward", "backward", "selected")

# PSNR (dB) of the t = 0.5 frame against the rendered true mid-frame, measured with table_row below (float64 witness of the
# estimator run both ways, project64, select_f32): MEASURED[(warps, median, rounds)][row of W.ROWS] = (forward-only,
# backward-only, selected).  tests/test_flow_select_yardstick.py holds every cell to these figures minus 0.05 dB; DESIGN section
# 8.1 quotes them.
MEASURED = {
    (1, 0, 0): [
        (31.85, 31.40, 32.76),
        (32.15, 31.25, 32.92),
        (27.68, 27.70, 28.36),
        (34.16, 34.11, 36.14),
        (26.44, 26.87, 26.93),
        (26.07, 25.55, 26.79),
        (23.35, 23.06, 23.41),
    ],
    (1, 0, 3): [
        (31.93, 31.82, 32.60),
        (33.23, 32.53, 34.10),
        (27.83, 27.78, 28.33),
        (35.04, 35.22, 35.86),
        (26.46, 26.91, 27.01),
        (26.62, 26.33, 27.22),
        (23.68, 23.47, 24.03),
    ],
    (2, 5, 0): [
        (34.43, 34.25, 35.72),
        (34.22, 33.93, 35.75),
        (29.90, 30.42, 30.90),
        (36.16, 35.65, 38.26),
        (28.07, 29.66, 29.36),
        (28.87, 28.36, 29.89),
        (23.89, 23.75, 24.02),
    ],
    (2, 5, 3): [
        (34.63, 34.50, 35.43),
        (36.05, 35.60, 36.51),
        (30.12, 30.54, 30.76),
        (37.47, 37.11, 37.58),
        (28.16, 29.66, 29.61),
        (29.52, 29.23, 29.87),
        (24.24, 24.05, 24.25),
    ],
}


def _samples(a, b, g, t):
    h, w = a.shape[:2]
    one = _f(1.0)
    nt = one - t
    xs = np.arange(w, dtype=_f)[None, :].repeat(h, 0)
    ys = np.arange(h, dtype=_f)[:, None].repeat(w, 1)
    sa = oracle_np._sample_trunc(a, xs - t * g[..., 0], ys - t * g[..., 1]).astype(_f)
    sb = oracle_np._sample_trunc(b, xs + nt * g[..., 0], ys + nt * g[..., 1]).astype(_f)
    return sa, sb


def _error(sa, sb):
    d = np.abs(sa[..., :3] - sb[..., :3])
    e = (d[..., 0] + d[..., 1]) + d[..., 2]
    assert e.dtype == _f
    return e


def candidates_f32(F, R, t, rounds):
    """(gF, gR) in float32: the two vectors of every output pixel."""
    t = _f(t)
    nt = _f(1.0) - t
    return PJ.project_f32(F, t, rounds), -PJ.project_f32(R, nt, rounds)


def select_from(a, b, gF, gR, t):
    """The choice and the frame from the two candidate fields (float32)."""
    t = _f(t)
    nt = _f(1.0) - t
    saF, sbF = _samples(a, b, gF, t)
    saR, sbR = _samples(a, b, gR, t)
    eF, eR = _error(saF, sbF), _error(saR, sbR)
    back = eR < eF
    sa = np.where(back[..., None], saR, saF)
    sb = np.where(back[..., None], sbR, sbF)
    return oracle_np._as_u8_trunc(nt * sa + t * sb), back, eF, eR


def select_f32(a, b, F, R, t, rounds):
    """-> (frame (h, w, 4) uint8, picked_backward (h, w) bool, eF, eR (h, w) float32 integers 0 .. 765)."""
    F, R = np.asarray(F, _f), np.asarray(R, _f)
    if F.shape != a.shape[:2] + (2,) or R.shape != F.shape or a.shape != b.shape:
        raise ValueError("frames / flows")
    gF, gR = candidates_f32(F, R, t, rounds)
    return select_from(a, b, gF, gR, t)


def _sample_loop(frame, x, y):
    h, w = frame.shape[:2]
    x = min(max(x, _f(0)), _f(w - 1))
    y = min(max(y, _f(0)), _f(h - 1))
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    xf, yf = x - _f(x0), y - _f(y0)
    one = _f(1.0)
    out = np.empty(4, _f)
    for c in range(4):
        top = _f(frame[y0, x0, c]) * (one - xf) + _f(frame[y0, x1, c]) * xf
        bottom = _f(frame[y1, x0, c]) * (one - xf) + _f(frame[y1, x1, c]) * xf
        out[c] = min(max(np.trunc(top * (one - yf) + bottom * yf), _f(0)), _f(255))
    return out


def select_loop(a, b, F, R, t, rounds):
    """select_f32 as a literal per-pixel loop over scalars (the yardstick test compares the two)."""
    F, R = np.asarray(F, _f), np.asarray(R, _f)
    h, w = a.shape[:2]
    t = _f(t)
    one = _f(1.0)
    nt = one - t
    gF = PJ.project_loop(F, t, rounds)
    gR = PJ.project_loop(R, nt, rounds)
    frame = np.empty((h, w, 4), np.uint8)
    back = np.empty((h, w), bool)
    eF, eR = np.empty((h, w), _f), np.empty((h, w), _f)
    for y in range(h):
        for x in range(w):
            cand = []
            for g in (gF[y, x], -gR[y, x]):
                sa = _sample_loop(a, _f(x) - t * g[0], _f(y) - t * g[1])
                sb = _sample_loop(b, _f(x) + nt * g[0], _f(y) + nt * g[1])
                e = (abs(sa[0] - sb[0]) + abs(sa[1] - sb[1])) + abs(sa[2] - sb[2])
                cand.append((e, sa, sb))
            eF[y, x], eR[y, x] = cand[0][0], cand[1][0]
            back[y, x] = cand[1][0] < cand[0][0]
            _, sa, sb = cand[1] if back[y, x] else cand[0]
            for c in range(4):
                frame[y, x, c] = int(min(max(np.trunc(nt * sa[c] + t * sb[c]), _f(0)), _f(255)))
    return frame, back, eF, eR


# ---- FMA mode: which pixels, as a whole, the warp contract admits for a given vector field ----------------------------------------------
def _banded_candidates(img, p_x, p_y, coef, flow, position_ulps, flow_band):
    """_warp64._candidates for a flow known to `flow_band` px per component only: the position p + coef flow moves by up to
    |coef| flow_band on each axis, and the bilinear sample, continuous and of slope at most 255 counts per pixel on each axis, by
    255 times that.  An axis clamps to a border only where the position is beyond it by more than that reach."""
    import _warp64 as C

    if flow_band == 0.0:
        return C._candidates(img, p_x, p_y, coef, flow, position_ulps)
    h, w = img.shape[:2]
    reach = abs(coef) * flow_band

    def axis(p, f, n):
        x, e = C._axis(p, coef, f, n, position_ulps)  # (e is 0 outside [0, n - 1])
        raw = p + coef * f
        return x, np.where((raw <= -reach) | (raw >= n - 1.0 + reach), e, e + reach)

    x, ex = axis(p_x, flow[..., 0], w)
    y, ey = axis(p_y, flow[..., 1], h)
    s = C.warp_samples64(img, x, y)
    eps = (255.0 * (ex + ey) + C.ARITH_BAND)[..., None]
    exact = ((ex == 0.0) & (ey == 0.0) & (x * 256.0 == np.floor(x * 256.0)) & (y * 256.0 == np.floor(y * 256.0)))[..., None]
    lo = np.floor(s)
    return s, lo, ~exact & (s - lo <= eps) & (lo >= 1.0), ~exact & (lo + 1.0 - s <= eps) & (lo <= 254.0)


def contract_pixels(got, a, b, flow, t, position_ulps, flow_band=0.0):
    """(h, w) bool: the pixels of uint8 `got` (h, w, 4) whose four bytes all meet the FMA warp contract of tests/_warp64.py with
    `flow` (h, w, 2) as the pair's flow at time t -- each byte is trunc(f32(nt sa) + f32(t sb)) for a pair of sample counts the
    contract admits (floor(s), or a neighbouring integer where the float64 sample s is within its error band of it).
    flow_band (px, absolute): the warp's flow is `flow` to within that much per component (an estimator mode's stated bound); the
    error band of each sample widens by 255 counts per pixel of it and axis.  0: the contract as it is."""
    import _warp64 as C

    h, w = a.shape[:2]
    t32 = _f(t)
    nt32 = _f(1.0) - t32
    p_x = np.arange(w, dtype=np.float64)[None, :]
    p_y = np.arange(h, dtype=np.float64)[:, None]
    fl = np.asarray(flow).astype(np.float64)
    _, lo_a, below_a, above_a = _banded_candidates(a, p_x, p_y, -float(t32), fl, position_ulps, float(flow_band))
    _, lo_b, below_b, above_b = _banded_candidates(b, p_x, p_y, float(nt32), fl, position_ulps, float(flow_band))
    g = got.astype(_f)
    ok = g == C._blend32(lo_a, lo_b, t32, nt32)
    for d_a, m_a in ((0.0, None), (-1.0, below_a), (1.0, above_a)):
        for d_b, m_b in ((0.0, None), (-1.0, below_b), (1.0, above_b)):
            if m_a is None and m_b is None:
                continue
            m = m_b if m_a is None else m_a if m_b is None else m_a & m_b
            ok |= m & (g == C._blend32(lo_a + d_a, lo_b + d_b, t32, nt32))
    return ok.all(axis=-1)


# ---- the quality table -------------------------------------------------------------------------------------------------------------
def witness_flows(row, warps, median):
    """The float64 witness estimator's flows of a table scene, A -> B and B -> A, rounded to float32 (what the warp reads)."""
    a, b, _ = W.scene(row)
    fwd = M.estimate(a, b, warps=warps, median=median, **W.PARAMS).astype(_f)
    bwd = M.estimate(b, a, warps=warps, median=median, **W.PARAMS).astype(_f)
    return fwd, bwd


def table_row(row, settings=SETTINGS, rounds=ROUNDS):
    """-> {(warps, median, rounds): (forward-only, backward-only, selected) PSNR (dB) of the t = 0.5 frame against the scene's true
    mid-frame}.  The candidates are project64's, rounded to float32 as the projection table's are."""
    a, b, mid = W.scene(row)
    out = {}
    for wn, med in settings:
        F, R = witness_flows(row, wn, med)
        for n in rounds:
            gF = PJ.project64(F, 0.5, n).astype(_f)
            gR = (-PJ.project64(R, 0.5, n)).astype(_f)
            sel = select_from(a, b, gF, gR, 0.5)[0]
            out[wn, med, n] = (scenes.psnr_rgb(oracle_np.warp_blend(a, b, gF, 0.5), mid),
                               scenes.psnr_rgb(oracle_np.warp_blend(a, b, gR, 0.5), mid), scenes.psnr_rgb(sel, mid))
    return out


def format_table(rows, settings=SETTINGS, rounds=ROUNDS):
    """Forward-only in dB, then backward-only and selected as gains over it."""
    cols = [(wn, med, n) for wn, med in settings for n in rounds]
    head = " | ".join(f"warps {wn}, median {med}, rounds {n}: forward (dB) | backward | selected" for wn, med, n in cols)
    out = ["| w×h, pan, square motion (square side) | " + head + " |", "|---|" + "---|" * (3 * len(cols))]
    for row, psnr in rows:
        w, h, pan, mv, sq = row
        cells = []
        for col in cols:
            fwd, bwd, sel = psnr[col]
            cells += [f"{fwd:.2f}", f"{bwd - fwd:+.2f}", f"{sel - fwd:+.2f}"]
        out.append(f"| {w}×{h}, ({pan[0]},{pan[1]}), ({mv[0]},{mv[1]}) ({sq}) | " + " | ".join(cells) + " |")
    return "\n".join(out)
