"""Yardstick of the forward-backward block-matching mode (nus_bm_set_bidirectional of include/nuscaler_hip.h, "Forward-backward
check"): the consistency rule, the choice and the fill in plain numpy integers on top of tests/_blockmatch.py, the synthetic
scene with a known true mid-frame, and the quality table DESIGN section 8.5 quotes.  Written for the tests;
test_bm_bidir_yardstick.py checks `repair` against a literal per-block loop."""
import numpy as np

import _blockmatch as bmref

NO_MATCH = bmref.NO_MATCH
DEFAULT_TOLERANCE = 2  # NUS_BM_BIDIR_DEFAULT_TOLERANCE
FROM_BACKWARD, FILLED, NO_NEIGHBOUR = 4, 8, 16  # flag bits 2, 3, 4
_LAST = 1 << 20  # sorts behind every vector component


def smooth_noise(rng, H, W, k=3):
    x = rng.integers(0, 256, (H, W, 3)).astype(np.float64)
    for _ in range(k):
        x = (np.roll(x, 1, 0) + np.roll(x, -1, 0) + np.roll(x, 1, 1) + np.roll(x, -1, 1) + x) / 5
    x = (x - x.min()) / (x.max() - x.min()) * 255
    return x.astype(np.uint8)


def scene(w, h, pan, mv, sq=48, seed=1):
    """-> A, B, true mid-frame (h, w, 4) uint8: a smoothed-noise background that pans by `pan`, a textured square of side `sq`
    that moves over it by `mv`; pan and mv even, so the half step is a whole pixel."""
    rng = np.random.default_rng(seed)
    M = 64
    bg = smooth_noise(rng, h + 2 * M, w + 2 * M)
    fg = smooth_noise(rng, sq, sq, 1)

    def frame(f):  # f = 0, 1, 2 half steps
        ox, oy = M + pan[0] * f // 2, M + pan[1] * f // 2
        im = bg[oy:oy + h, ox:ox + w].copy()
        x0, y0 = 40 + mv[0] * f // 2, 30 + mv[1] * f // 2
        im[y0:y0 + sq, x0:x0 + sq] = fg
        return np.dstack([im, np.full((h, w), 255, np.uint8)])

    return frame(0), frame(2), frame(1)


# the rows of the table: w, h, block size, radius, pan, square motion, square side
ROWS = [
    (192, 128, 8, 16, (-4, 2), (12, 4), 48),
    (192, 128, 16, 16, (-4, 2), (12, 4), 48),
    (192, 128, 8, 16, (0, 0), (12, 4), 48),
    (192, 128, 8, 24, (2, 0), (-20, 8), 48),
    (192, 128, 32, 8, (-4, 2), (6, -4), 48),
    (200, 72, 16, 16, (6, 0), (-10, 6), 32),
    (200, 72, 8, 24, (6, 0), (-10, 6), 32),
]


def consistent(P, sad_p, Q, sad_q, w, h, bs, tolerance):
    """(by, bx) bool: is the block of the P search consistent with the Q search (the same grid, frames exchanged)?"""
    nby, nbx = sad_p.shape
    p, q = P.astype(np.int64), Q.astype(np.int64)
    cx = np.clip(np.arange(nbx)[None, :] * bs + p[..., 0] + bs // 2, 0, w - 1) // bs
    cy = np.clip(np.arange(nby)[:, None] * bs + p[..., 1] + bs // 2, 0, h - 1) // bs
    g = q[cy, cx]
    return (sad_p != NO_MATCH) & (sad_q[cy, cx] != NO_MATCH) & (np.abs(p + g).sum(-1) <= tolerance)


def repair(F, sad_f, G, sad_g, w, h, bs, tolerance=DEFAULT_TOLERANCE):
    """F, G: (by, bx, 2) int16 raw winners of the search A -> B and B -> A; sad_*: (by, bx) uint32 -> (V int16, flags uint8)."""
    nby, nbx = sad_f.shape
    ok_a = consistent(F, sad_f, G, sad_g, w, h, bs, tolerance)
    ok_b = consistent(G, sad_g, F, sad_f, w, h, bs, tolerance)
    V = np.where(ok_a[..., None], F, -G).astype(np.int64)
    resolved = ok_a | ok_b
    flags = np.where(~ok_a & ok_b, FROM_BACKWARD, 0).astype(np.uint8)
    pad_v = np.full((nby + 2, nbx + 2, 2), _LAST, np.int64)
    pad_v[1:-1, 1:-1] = np.where(resolved[..., None], V, _LAST)
    near = np.stack([pad_v[1 + oy:1 + oy + nby, 1 + ox:1 + ox + nbx] for oy in (-1, 0, 1) for ox in (-1, 0, 1) if ox or oy])
    near = np.sort(near, axis=0)  # (8, by, bx, 2): each component on its own, the missing ones last
    n = (near[..., 0] != _LAST).sum(0)
    med = np.take_along_axis(near, np.broadcast_to((np.maximum(n, 1) - 1) // 2, (1, nby, nbx))[..., None].repeat(2, -1), 0)[0]
    med[n == 0] = 0
    V = np.where(resolved[..., None], V, med)
    flags[~resolved] = np.where(n[~resolved] > 0, FILLED, NO_NEIGHBOUR)
    return V.astype(np.int16), flags


def estimate(a, b, bs, R, order=bmref.CENTER, tolerance=DEFAULT_TOLERANCE):
    """-> dict of F, sad_f, G, sad_g, V, flags for the pair (a, b): what the mode computes, start to end."""
    h, w = a.shape[:2]
    F, sad_f = bmref.vectors(a, b, bs, R, order)
    G, sad_g = bmref.vectors(b, a, bs, R, order)
    V, flags = repair(F, sad_f, G, sad_g, w, h, bs, tolerance)
    return {"F": F, "sad_f": sad_f, "G": G, "sad_g": sad_g, "V": V, "flags": flags}


def psnr_rgb(x, y):
    d = x[..., :3].astype(np.float64) - y[..., :3].astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / (d * d).mean())


def table_row(warp_blend, row, tolerance=DEFAULT_TOLERANCE):
    """-> (PSNR raw winners, PSNR confidence-pass default, PSNR forward-backward, counts of flags 4 / 8 / 16, blocks) of the
    t = 0.5 frame against the scene's mid-frame; `warp_blend` is the oracle's."""
    w, h, bs, R, pan, mv, sq = row
    a, b, mid = scene(w, h, pan, mv, sq)
    e = estimate(a, b, bs, R, bmref.CENTER, tolerance)

    def quality(v):
        return psnr_rgb(warp_blend(a, b, bmref.dense_flow(v, w, h, bs), 0.5), mid)

    counts = tuple(int((e["flags"] == f).sum()) for f in (FROM_BACKWARD, FILLED, NO_NEIGHBOUR))
    return quality(e["F"]), quality(bmref.refine(e["F"])[0]), quality(e["V"]), counts, e["flags"].size


def format_table(rows):
    out = ["| w×h, bs / R, pan, square motion | raw winners | default (confidence pass) | forward-backward | flags 4 / 8 / 16 |",
           "|---|---|---|---|---|"]
    for row, (raw, default, bidir, counts, blocks) in rows:
        w, h, bs, R, pan, mv, sq = row
        name = f"{w}×{h}, {bs} / {R}, ({pan[0]},{pan[1]}), ({mv[0]},{mv[1]})" + (f" (square {sq})" if sq != 48 else "")
        out.append(f"| {name} | {raw:.2f} | {default:.2f} | **{bidir:.2f}** | {counts[0]} / {counts[1]} / {counts[2]} of {blocks} |")
    return "\n".join(out)
