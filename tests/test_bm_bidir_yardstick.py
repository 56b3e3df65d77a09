"""The yardstick of the forward-backward block-matching mode (tests/_bm_bidir.py) against a literal per-block loop and on
hand-made fields, and what the mode is for: on synthetic pairs with a known true mid-frame its t = 0.5 frame is at least 1 dB
nearer the truth than the raw winners' and than the confidence-pass default's.  No GPU."""
import functools

import numpy as np
import pytest

import _blockmatch as bmref
import _bm_bidir as bidir

NO_MATCH = bidir.NO_MATCH


def _clamp(v, lo, hi):
    return max(lo, min(hi, v))


def _loop_consistent(P, sp, Q, sq, bx, by, w, h, bs, tol):
    dx, dy = int(P[by, bx, 0]), int(P[by, bx, 1])
    cx = _clamp(bx * bs + dx + bs // 2, 0, w - 1) // bs
    cy = _clamp(by * bs + dy + bs // 2, 0, h - 1) // bs
    gx, gy = int(Q[cy, cx, 0]), int(Q[cy, cx, 1])
    return int(sp[by, bx]) != NO_MATCH and int(sq[cy, cx]) != NO_MATCH and abs(dx + gx) + abs(dy + gy) <= tol


def _loop_repair(F, sf, G, sg, w, h, bs, tol):
    """The header's steps 2 - 4, block by block."""
    nby, nbx = sf.shape
    V3 = np.zeros((nby, nbx, 2), np.int64)
    state = np.zeros((nby, nbx), np.int64)  # 0 forward, 4 backward, -1 unresolved
    for by in range(nby):
        for bx in range(nbx):
            if _loop_consistent(F, sf, G, sg, bx, by, w, h, bs, tol):
                V3[by, bx] = F[by, bx]
            elif _loop_consistent(G, sg, F, sf, bx, by, w, h, bs, tol):
                V3[by, bx] = (-int(G[by, bx, 0]), -int(G[by, bx, 1]))
                state[by, bx] = 4
            else:
                state[by, bx] = -1
    V, flags = V3.copy(), np.where(state < 0, 0, state).astype(np.uint8)
    for by in range(nby):
        for bx in range(nbx):
            if state[by, bx] >= 0:
                continue
            near = [V3[y, x] for y in range(by - 1, by + 2) for x in range(bx - 1, bx + 2)
                    if (x, y) != (bx, by) and 0 <= x < nbx and 0 <= y < nby and state[y, x] >= 0]
            if not near:
                V[by, bx], flags[by, bx] = (0, 0), 16
                continue
            for c in (0, 1):
                V[by, bx, c] = sorted(int(v[c]) for v in near)[(len(near) - 1) // 2]
            flags[by, bx] = 8
    return V.astype(np.int16), flags


@pytest.mark.parametrize("nbx,nby,bs,cut_w,cut_h", [(1, 1, 8, 0, 0), (1, 1, 8, 7, 7), (1, 6, 16, 3, 0), (7, 1, 8, 0, 5), (2, 2, 32, 0, 0),
                                                     (9, 5, 8, 3, 6), (13, 11, 16, 15, 1), (6, 4, 32, 0, 31)])
def test_vectorised_yardstick_equals_the_per_block_loop(nbx, nby, bs, cut_w, cut_h):
    w, h = nbx * bs - cut_w, nby * bs - cut_h  # partial blocks at the right and bottom edge
    rng = np.random.default_rng(100 * nbx + nby)
    seen = set()
    for trial in range(24):
        R = (2, 6, 24)[trial % 3]  # small radii make consistent pairs likely, 24 throws vectors over the frame border: the clamp
        F = rng.integers(-R, R + 1, (nby, nbx, 2)).astype(np.int16)
        G = rng.integers(-R, R + 1, (nby, nbx, 2)).astype(np.int16)
        if trial % 2:  # half of the trials: G mostly answers F, so that every kind of block occurs
            G = np.where(rng.random((nby, nbx, 1)) < 0.6, -F, G).astype(np.int16)
        sf = rng.integers(0, 1000, (nby, nbx)).astype(np.uint32)
        sg = rng.integers(0, 1000, (nby, nbx)).astype(np.uint32)
        sf[rng.random((nby, nbx)) < 0.15] = NO_MATCH
        sg[rng.random((nby, nbx)) < 0.15] = NO_MATCH
        for tol in (0, 2, 96):
            V, flags = bidir.repair(F, sf, G, sg, w, h, bs, tol)
            Vl, fl = _loop_repair(F, sf, G, sg, w, h, bs, tol)
            assert np.array_equal(flags, fl), (trial, tol)
            assert np.array_equal(V, Vl), (trial, tol)
            assert V.dtype == np.int16 and flags.dtype == np.uint8 and np.abs(V).max() <= 24
            seen |= set(flags.ravel().tolist())
    assert seen <= {0, 4, 8, 16}
    if nbx * nby > 4:
        assert seen == {0, 4, 8, 16}, seen


def _field(nbx, nby, v):
    F = np.empty((nby, nbx, 2), np.int16)
    F[...] = v
    return F, np.full((nby, nbx), 100, np.uint32)


def test_agreeing_fields_are_kept():
    F, s = _field(6, 4, (5, -3))
    V, flags = bidir.repair(F, s, (-F).astype(np.int16), s, 96, 64, 16, 0)
    assert np.array_equal(V, F) and not flags.any()


def test_one_wrong_forward_block_is_replaced_by_the_backward_vector():
    # (12, -10) at block size 16 carries a block's centre into the next block: B's block (3, 2) answers to A's block (2, 3), a
    # good one, not to the wrong block at its own position
    F, s = _field(6, 4, (12, -10))
    G = (-F).astype(np.int16)
    F[2, 3] = (-20, 11)
    V, flags = bidir.repair(F, s, G, s, 96, 64, 16, 2)
    want = np.zeros((4, 6), np.uint8)
    want[2, 3] = 4
    assert np.array_equal(flags, want)
    assert (V == (12, -10)).all()


def _unresolved_centre(near):
    """3 x 3 blocks of 8: the centre unresolved in both directions, neighbour k resolved with vector near[k] or, where near[k] is
    None, unresolved too.  Neighbours in row-major order without the centre."""
    F, G = np.zeros((3, 3, 2), np.int16), np.zeros((3, 3, 2), np.int16)
    s = np.full((3, 3), 7, np.uint32)
    sf = s.copy()
    cells = [(y, x) for y in range(3) for x in range(3) if (y, x) != (1, 1)]
    for (y, x), v in zip(cells, near):
        if v is None:
            sf[y, x] = NO_MATCH  # forward: no match; backward: G = 0 lands on this block itself, whose forward SAD is no match
        else:
            F[y, x], G[y, x] = v, (-v[0], -v[1])  # |v| <= 3 < bs / 2: each lands on its own block and agrees
    sf[1, 1] = NO_MATCH
    return bidir.repair(F, sf, G, s, 24, 24, 8, 0)


def test_fill_takes_the_lower_median_per_component():
    near = [(3, -1), (1, 2), (-2, 0), (0, 3), (2, -3), (-1, 1), (-3, -2), (1, 0)]
    V, flags = _unresolved_centre(near)
    assert flags[1, 1] == 8 and (np.delete(flags.ravel(), 4) == 0).all()
    # dx sorted: -3 -2 -1 0 1 1 2 3 -> element (8 - 1) // 2 = 3 -> 0; dy sorted: -3 -2 -1 0 0 1 2 3 -> 0
    assert tuple(V[1, 1]) == (0, 0)
    near = [(3, -1), (1, 2), (-2, 1), (2, 3), (2, -3), (-1, 1), (-3, -2), (3, 2)]
    V, flags = _unresolved_centre(near)
    # dx: -3 -2 -1 1 2 2 3 3 -> 1 (the upper median would be 2); dy: -3 -2 -1 1 1 2 2 3 -> 1
    assert flags[1, 1] == 8 and tuple(V[1, 1]) == (1, 1)
    near = [None, (3, -2), None, None, (-1, 3), (2, 0), None, None]
    V, flags = _unresolved_centre(near)
    # three resolved neighbours: dx -1 2 3 -> element 1 -> 2; dy -2 0 3 -> 0
    assert flags[1, 1] == 8 and tuple(V[1, 1]) == (2, 0)
    near = [None, (3, -2), None, None, (-1, 3), None, None, None]
    V, flags = _unresolved_centre(near)
    # an even count, two: element (2 - 1) // 2 = 0, the smaller of each component
    assert flags[1, 1] == 8 and tuple(V[1, 1]) == (-1, -2)


def test_nothing_resolved_gives_zero_vectors_and_flag_16():
    rng = np.random.default_rng(3)
    F = rng.integers(-24, 25, (5, 7, 2)).astype(np.int16)
    G = rng.integers(-24, 25, (5, 7, 2)).astype(np.int16)
    s = np.full((5, 7), NO_MATCH, np.uint32)
    V, flags = bidir.repair(F, s, G, s, 7 * 8, 5 * 8, 8, 96)
    assert (flags == 16).all() and not V.any()
    # one block, nothing admitted: the 1 x 1 frame of the device tests
    a = np.zeros((1, 1, 4), np.uint8)
    e = bidir.estimate(a, a, 8, 1)
    assert e["sad_f"][0, 0] == NO_MATCH and e["flags"][0, 0] == 16 and not e["V"].any()


@functools.lru_cache(maxsize=None)
def _table(warp_blend):
    return tuple((row, bidir.table_row(warp_blend, row)) for row in bidir.ROWS)


def test_quality_against_the_true_mid_frame(oracle_mod):
    rows = _table(oracle_mod.warp_blend)
    print()
    print(bidir.format_table(rows))
    for row, (raw, default, fb, counts, blocks) in rows:
        print(f"{row}: gain over raw {fb - raw:.2f} dB, over default {fb - default:.2f} dB")
    for row, (raw, default, fb, counts, blocks) in rows:
        assert fb >= raw + 1.0, (row, raw, fb)
        assert fb >= default + 1.0, (row, default, fb)
        assert counts[2] == 0 and sum(counts) <= blocks
