"""Float64 yardstick for the FMA mode of the resize kernels (Lanczos-3 / Catmull-Rom / Triangle).

The contract: let v be the resample accumulated in float64 from the oracle's own f32 tap weights
(oracle.resize_axis), c = clip(v, 0, 255).  An FMA-mode output sample equals floor(c + 0.5); where c lies within eps of a
rounding tie (|c - floor(c) - 0.5| <= eps) it may also be the other neighbour.  That is what a kernel that accumulates in f32
and rounds to nearest (either tie rule) produces, whatever the order of its sums; it fails a kernel that truncates, adds a
bias, or whose weights drift by 1e-5 relative.  The weights come from the oracle, not from the product's tables, so the
yardstick stays independent of nus_tables.cpp (tests/test_oracle_witness.py pins them to the closed-form kernels).

eps = 1e-3 * max(1, (Tx + Ty) / 12) LSB, Tx and Ty the widest tap windows of the two axes: the f32 accumulation error of
one pass is about 2^-24 * 330 per tap, so the band grows with the tap count (about 5e-3 for 32-tap down-scaling windows).
"""
import numpy as np

EPS_BASE = 1e-3
_CHUNK_SAMPLES = 1 << 21  # float64 samples per row chunk of the horizontal pass (16 MiB): a 4K reference stays small


def eps_rule(tx: int, ty: int) -> float:
    """The tie band for widest tap windows tx (horizontal) and ty (vertical)."""
    return EPS_BASE * max(1.0, (tx + ty) / 12.0)


def _axis(oracle_mod, in_n, out_n, filt):
    left, ntaps, w = oracle_mod.resize_axis(in_n, out_n, filt)
    taps = int(ntaps.max())
    return left.astype(np.int64), taps, w[:, :taps].astype(np.float64)


def contract_eps(oracle_mod, iw, ih, ow, oh, filt) -> float:
    """eps_rule for a resize of (iw, ih) to (ow, oh) with filter `filt`."""
    return eps_rule(_axis(oracle_mod, iw, ow, filt)[1], _axis(oracle_mod, ih, oh, filt)[1])


def resample64(oracle_mod, img, ow, oh, filt):
    """The resample of one (h, w, 4) uint8 frame to (oh, ow, 4) in float64: vertical pass, then horizontal, with the oracle's
    f32 tap weights.  Banded: loops over taps and over chunks of output rows, never a (rows, taps, width, 4) array."""
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] == 4 and img.dtype == np.uint8, img.shape
    ih, iw = img.shape[:2]
    if (iw, ih) == (ow, oh):  # imageops::resize returns a copy when the dimensions are unchanged (so does the oracle)
        return img.astype(np.float64)
    ly, ty, wy = _axis(oracle_mod, ih, oh, filt)
    lx, tx, wx = _axis(oracle_mod, iw, ow, filt)
    src = img.astype(np.float64)
    out = np.empty((oh, ow, 4), np.float64)
    rows = max(1, _CHUNK_SAMPLES // (4 * max(iw, ow)))
    for y0 in range(0, oh, rows):
        y1 = min(oh, y0 + rows)
        tmp = np.zeros((y1 - y0, iw, 4), np.float64)
        for i in range(ty):  # (slots beyond a window's taps hold weight 0; their clipped index reads a real row)
            tmp += wy[y0:y1, i, None, None] * src[np.minimum(ly[y0:y1] + i, ih - 1)]
        acc = out[y0:y1]
        acc.fill(0.0)
        for j in range(tx):
            acc += wx[None, :, j, None] * tmp[:, np.minimum(lx + j, iw - 1)]
    return out


def _parts(got, v):
    """got as float64, floor(c + 0.5), floor(c) and the tie distance |c - floor(c) - 0.5| per sample."""
    got = np.asarray(got)
    assert got.shape == v.shape, (got.shape, v.shape)
    c = np.clip(v, 0.0, 255.0)
    lo = np.floor(c)
    ref = np.floor(c + 0.5)
    tie = np.abs(c - lo - 0.5)
    return got.astype(np.float64), ref, lo, tie


def assert_fma_contract(got, v, eps, tag):
    """Assert the FMA contract for uint8 `got` against float64 `v` (same shape: (h, w, 4) or (frames, h, w, 4)).  Returns
    {"samples", "differ", "worst_tie"}: how many samples differ from floor(c + 0.5) and the largest tie distance among them."""
    g, ref, lo, tie = _parts(got, v)
    near_tie = tie <= eps
    ok = (g == ref) | (near_tie & ((g == lo) | (g == lo + 1)))
    differ = g != ref
    worst = float(tie[differ].max()) if differ.any() else None
    far = np.abs(g - ref) > 1
    if not ok.all() or far.any():
        bad = np.argwhere(~ok)
        if bad.shape[1] == 3:
            bad = np.concatenate([np.zeros((len(bad), 1), bad.dtype), bad], axis=1)
        vv = v if v.ndim == 4 else v[None]
        gg = got if got.ndim == 4 else got[None]
        first = [(tuple(int(k) for k in idx), float(vv[tuple(idx)]), int(gg[tuple(idx)])) for idx in bad[:6]]
        raise AssertionError(
            f"FMA contract violated ({tag}): {int((~ok).sum())} of {ok.size} samples not floor(c + 0.5) outside the tie band "
            f"eps={eps:.3g}, {int(far.sum())} more than 1 LSB away; first (frame, y, x, channel), v, got: {first}; "
            f"worst tie distance among the {int(differ.sum())} differing samples: {worst}")
    return {"samples": int(g.size), "differ": int(differ.sum()), "worst_tie": worst}


def check_fma(oracle_mod, got, src, ow, oh, filt, tag):
    """resample64 + contract_eps + assert_fma_contract for one frame `src` (h, w, 4) or a stack of frames (n, h, w, 4)."""
    src = np.asarray(src)
    frames = src if src.ndim == 4 else src[None]
    ih, iw = frames.shape[1:3]
    v = np.stack([resample64(oracle_mod, f, ow, oh, filt) for f in frames])
    if src.ndim == 3:
        v = v[0]
    return assert_fma_contract(got, v, contract_eps(oracle_mod, iw, ih, ow, oh, filt), tag)
