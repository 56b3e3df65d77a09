"""tests/_blockmatch.py against a literal restatement of the reference's per-block, per-candidate, per-pixel loops
(find_best_match, nu_scaler_core/src/interpolation/mod.rs:584-622, and calculate_sad, :555-581) on tiny frames, and its integer
confidence rule against the reference's f32 expression.  No GPU."""
import numpy as np
import pytest

import _blockmatch as bmref


def literal(a, b, bs, R, order):
    h, w = a.shape[:2]
    nbx, nby = -(-w // bs), -(-h // bs)
    mv = np.zeros((nby, nbx, 2), np.int16)
    sad = np.full((nby, nbx), bmref.NO_MATCH, np.uint32)
    cands = [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    if order == bmref.CENTER:
        cands = sorted(cands, key=lambda v: v[0] ** 2 + v[1] ** 2)
    for by in range(nby):
        for bx in range(nbx):
            x0, y0 = bx * bs, by * bs
            best = None
            for dx, dy in cands:
                if x0 + dx < 0 or x0 + dx + bs > w or y0 + dy < 0 or y0 + dy + bs > h:
                    continue
                s = 0
                for y in range(bs):
                    for x in range(bs):
                        if x0 + x >= w or y0 + y >= h:
                            continue
                        for c in range(3):  # alpha is skipped (:572-576)
                            s += abs(int(a[y0 + y, x0 + x, c]) - int(b[y0 + y + dy, x0 + x + dx, c]))
                if best is None or s < best:  # strict: the first minimum wins
                    best = s
                    mv[by, bx] = (dx, dy)
            if best is not None:
                sad[by, bx] = best
    return mv, sad


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


@pytest.mark.parametrize("order", [bmref.SCAN, bmref.CENTER])
@pytest.mark.parametrize("w,h,bs,R", [(16, 16, 8, 2), (13, 11, 8, 3), (5, 7, 8, 2), (1, 9, 8, 1), (12, 1, 8, 2), (1, 1, 8, 1),
                                      (20, 18, 16, 2), (17, 16, 16, 1), (33, 32, 32, 1)])
def test_search_equals_the_literal_loops(w, h, bs, R, order):
    a = noise(w, h, 1)
    b = np.roll(a, (1, -1), (0, 1)) if w > 2 and h > 2 else noise(w, h, 2)
    b[..., 3] = 255 - a[..., 3]  # alpha must not matter
    mv, sad = bmref.vectors(a, b, bs, R, order)
    lmv, lsad = literal(a, b, bs, R, order)
    assert np.array_equal(mv, lmv)
    assert np.array_equal(sad, lsad)


def test_frames_smaller_than_a_block_admit_nothing():
    a, b = noise(5, 7, 3), noise(5, 7, 4)
    mv, sad = bmref.vectors(a, b, 8, 4)
    assert not mv.any() and (sad == bmref.NO_MATCH).all()


def test_partial_edge_blocks_get_vectors():
    a = noise(40, 24, 5)
    b = np.roll(a, (0, 2), (0, 1))
    mv, sad = bmref.vectors(a, b, 16, 8)
    assert mv.shape == (2, 3, 2)
    # 8 pixels wide / high: the candidates that pull the whole block back inside frame B (dx <= -8 / dy <= -8) are admitted
    assert (sad[:, 2] != bmref.NO_MATCH).all() and (sad[1, :] != bmref.NO_MATCH).all()
    assert (mv[:, 2, 0] <= -8).all() and (mv[1, :, 1] <= -8).all()
    assert (bmref.vectors(a, b, 16, 7)[1][:, 2] == bmref.NO_MATCH).all()


def test_tie_orders_on_flat_frames():
    a = np.full((64, 64, 4), 100, np.uint8)
    for bs, R in ((16, 16), (8, 24), (32, 8)):
        scan, _ = bmref.vectors(a, a, bs, R, bmref.SCAN)
        center, sad = bmref.vectors(a, a, bs, R, bmref.CENTER)
        inner = [(by, bx) for by in range(64 // bs) for bx in range(64 // bs)
                 if bx * bs - R >= 0 and by * bs - R >= 0 and bx * bs + bs + R <= 64 and by * bs + bs + R <= 64]
        for by, bx in inner:
            assert tuple(scan[by, bx]) == (-R, -R)
        assert not center.any() and not sad.any()
    scan, _ = bmref.vectors(a, a, 16, 16, bmref.SCAN)
    assert tuple(scan[1, 1]) == (-16, -16)


def test_integer_confidence_rule_is_the_f32_expression():
    for total in range(0, 401):
        avg = np.float32(total) / np.float32(8.0)
        conf = np.float32(1.0) / (np.float32(1.0) + np.float32(0.1) * avg)
        assert bool(conf < np.float32(0.7)) == bool(bmref.confidence_cut(total)), total


def test_refine_rules():
    mv = np.zeros((5, 6, 2), np.int16)
    out, flags, smooth = bmref.refine(mv)
    assert smooth and not flags.any() and np.array_equal(out, mv)
    mv[:, 0] = (24, 24)  # column 0 and row 0 are never compared from their own side ...
    mv[0, :] = (-24, 24)
    mv[1:, 1:] = (3, -2)
    assert not bmref.refine(mv)[2]  # ... but block (1, 1) sees them as its left / top neighbour
    mv[:] = (3, -2)
    mv[2, 3] = (15, -2)  # one outlier: L1 12 to each of its 8 neighbours, 96 in all
    out, flags, smooth = bmref.refine(mv)
    assert not smooth and (flags & 2).all()
    assert tuple(out[2, 3]) == (0, 0) and flags[2, 3] == 3
    assert (flags & 1).sum() == 1  # each neighbour sums to 12: kept
    assert np.array_equal(out[flags & 1 == 0], mv[flags & 1 == 0])
