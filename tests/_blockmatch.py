"""Yardstick of the block-matching tests: the search, the confidence pass and the flow expansion of include/nuscaler_hip.h's
"Block-matching motion estimator" section in plain numpy integers (the search of nu_scaler_core/src/interpolation/mod.rs:555-622,
the pass of :795-910).  Written for the tests; test_blockmatch_yardstick.py checks it against a literal triple loop.

The search loops over candidates and sums each |A - shifted B| image per block: 320 x 240 at High takes a few seconds."""
import numpy as np

NO_MATCH = 0xFFFFFFFF
SCAN, CENTER = "scan", "center"


def candidates(R, order):
    """[(dx, dy)] in tie order: first in the list wins among equal SADs."""
    c = [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]  # dy outer, dx inner, ascending
    if order == CENTER:
        c.sort(key=lambda v: v[0] * v[0] + v[1] * v[1])  # stable: scan order among equal distances
    elif order != SCAN:
        raise ValueError(order)
    return c


def vectors(a, b, bs, R, order=CENTER):
    """a, b: (h, w, 4) uint8 -> (vectors int16 (by, bx, 2) as (dx, dy), sad uint32 (by, bx))."""
    h, w = a.shape[:2]
    nbx, nby = -(-w // bs), -(-h // bs)
    A, B = a[..., :3].astype(np.int64), b[..., :3].astype(np.int64)
    best = np.full((nby, nbx), np.iinfo(np.int64).max, np.int64)
    mv = np.zeros((nby, nbx, 2), np.int16)
    X0, Y0 = np.arange(nbx) * bs, np.arange(nby) * bs
    for dx, dy in candidates(R, order):
        okx = (X0 + dx >= 0) & (X0 + dx + bs <= w)
        oky = (Y0 + dy >= 0) & (Y0 + dy + bs <= h)
        if not okx.any() or not oky.any():
            continue
        d = np.zeros((nby * bs, nbx * bs), np.int64)  # zero beyond frame A: only A-side pixels inside the frame count
        ys0, ys1, xs0, xs1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        d[ys0:ys1, xs0:xs1] = np.abs(A[ys0:ys1, xs0:xs1] - B[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]).sum(-1)
        s = d.reshape(nby, bs, nbx, bs).sum((1, 3))  # (an admitted candidate's block lies inside d's filled part)
        better = (oky[:, None] & okx[None, :]) & (s < best)
        best[better] = s[better]
        mv[better] = (dx, dy)
    sad = np.where(best == np.iinfo(np.int64).max, NO_MATCH, best).astype(np.uint32)
    return mv, sad


def confidence_cut(total):
    """The integer form of the reference's 1 / (1 + 0.1 * sum / 8) < 0.7."""
    return total >= 35


def refine(mv):
    """-> (vectors after the confidence pass, flags uint8 (bit 0 zeroed, bit 1 pair not smooth), smooth)."""
    v = mv.astype(np.int64)
    nby, nbx = v.shape[:2]
    left = np.abs(v[1:, 1:] - v[1:, :-1]).sum(-1)
    top = np.abs(v[1:, 1:] - v[:-1, 1:]).sum(-1)
    smooth = not ((left > 10).any() or (top > 10).any())
    out = mv.copy()
    flags = np.zeros((nby, nbx), np.uint8)
    if smooth:
        return out, flags, True
    flags |= 2
    if nby > 2 and nbx > 2:
        total = np.zeros((nby - 2, nbx - 2), np.int64)
        c = v[1:-1, 1:-1]
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                if ox or oy:
                    total += np.abs(c - v[1 + oy:nby - 1 + oy, 1 + ox:nbx - 1 + ox]).sum(-1)
        cut = confidence_cut(total)
        out[1:-1, 1:-1][cut] = 0
        flags[1:-1, 1:-1][cut] |= 1
    return out, flags, False


def dense_flow(mv, w, h, bs):
    """(h, w, 2) float32: every pixel its block's (dx, dy)."""
    return np.repeat(np.repeat(mv, bs, axis=0), bs, axis=1)[:h, :w].astype(np.float32)
