"""Frame pairs chosen to break an SSIM kernel's arithmetic, shared by tests/test_metrics_reference.py (the CPU restatement of the
kernel against the float64 definition) and tests/test_gpu_metrics.py (the kernel itself), and the tolerance both assert.  Test
infrastructure only.

On noise the f32 rounding errors of the per-window statistics average out over the windows.  Here every window sees the same few
values, so whatever one window loses the mean loses: constant frames, stripes and checkerboards of two levels, letterbox bars.
The tile-edge shapes are the opposite kind: independent noise, whose window values spread over [0, 1], at sizes so small that
one wrong, missing or doubled window at a tile junction moves the mean by 1e-4 or more.

Every generator returns (name, A, B) with A, B uint8 arrays (N, H, W, 4); witness() is the float64 SSIM of each pair, computed
once per process."""
import functools

import numpy as np

import _metrics64 as M64

# The asserted SSIM tolerance: 4 x the worst |ssim_kernel_model - _metrics64.ssim| over every class below and over the SHAPES x
# CONTENTS of tests/test_gpu_metrics.py (measured: 1.31e-7, on the stripes; rounded up to two digits here; per class: that
# module's docstring).  The factor covers one ulp of the
# f32 divide and another libm, the margin tests/test_flow_witness.py takes.  The public contract stays 1e-5.
SSIM_MODEL_WORST = 1.4e-7
SSIM_TOL = 4 * SSIM_MODEL_WORST

CONST_W, CONST_H = 24, 20
PERIODIC_SIZES = [(30, 28), (139, 75)]
LEVELS = [(0, 1), (254, 255), (0, 255), (3, 252), (127, 128)]
# the SSIM tile is 64 x 32 centres plus a 5-pixel halo: one tile exactly, one more column and / or row of centres, two tiles
# each way exactly and one more, and the thinnest frames
TILE_EDGE_SHAPES = [(74, 42), (75, 42), (74, 43), (75, 43), (138, 74), (139, 75), (11, 200), (200, 11), (12, 11), (11, 12)]


def constant_pair_levels():
    """(c, d): d = c + 1, c - 1, c - 2, c + 5 for c = 0..255 where d is a level: 1015 pairs."""
    return [(c, c + k) for c in range(256) for k in (1, -1, -2, 5) if 0 <= c + k <= 255]


def _rgba(r, g, b, alpha):
    return np.stack([r, g, b, np.full_like(r, alpha)], axis=-1).astype(np.uint8)


def constant_pairs(per_channel=False):
    """The 1015 pairs as 24 x 20 frames.  per_channel: R = c, G = 255 - c, B = 128 against R = d, G = 255 - d, B = 128 + d - c, so
    that a slip in one channel cannot hide behind the other two."""
    cd = np.array(constant_pair_levels(), np.int64)
    c = np.broadcast_to(cd[:, 0, None, None], (len(cd), CONST_H, CONST_W))
    d = np.broadcast_to(cd[:, 1, None, None], (len(cd), CONST_H, CONST_W))
    if per_channel:
        return _rgba(c, 255 - c, np.full_like(c, 128), 7), _rgba(d, 255 - d, 128 + d - c, 200)
    return _rgba(c, c, c, 7), _rgba(d, d, d, 200)


def _periodic(kind, period, lo, hi, w, h):
    y, x = np.mgrid[0:h, 0:w]
    phase = {"vstripes": x, "hstripes": y, "checker": x + y}[kind]
    return np.where(phase % period == 0, hi, lo)


def periodic_pairs(w, h):
    """Stripes and checkerboards of two levels, period 2 and 3, each against itself one level up (down where the upper level is
    255), against itself rolled by one pixel across the pattern, and against the constant lower level.  -> (names, A, B)"""
    names, A, B = [], [], []
    for kind in ("vstripes", "hstripes", "checker"):
        for period in (2, 3):
            for lo, hi in LEVELS:
                a = _periodic(kind, period, lo, hi, w, h)
                others = {"level": a + 1 if hi < 255 else np.maximum(a - 1, 0),
                          "rolled": np.roll(a, 1, axis=0 if kind == "hstripes" else 1),
                          "constant": np.full_like(a, lo)}
                for what, b in others.items():
                    names.append(f"{kind}/{period}/{lo}-{hi}/{what}")
                    A.append(_rgba(a, a, a, 255))
                    B.append(_rgba(b, b, b, 0))
    return names, np.stack(A), np.stack(B)


def letterbox_pairs():
    """128 x 96: bars of level 16, 20 rows above and below a noise picture; the second frame has the same picture and bars of 17
    (black after a range conversion).  Then the same pair transposed: 96 x 128 with pillars.  -> two (A, B) of one pair each"""
    rng = np.random.default_rng(1617)
    a = rng.integers(0, 256, (96, 128, 4), dtype=np.int64)
    b = a.copy()
    for rows in (slice(0, 20), slice(76, 96)):
        a[rows, :, :3], b[rows, :, :3] = 16, 17
    a, b = a.astype(np.uint8), b.astype(np.uint8)
    return [("letterbox", a[None], b[None]),
            ("pillarbox", np.ascontiguousarray(a.transpose(1, 0, 2))[None], np.ascontiguousarray(b.transpose(1, 0, 2))[None])]


def tile_edge_triple(w, h):
    """Three pairs of independent noise frames of one size (the tests compare the middle one alone and inside the batch)."""
    rng = np.random.default_rng(1000 * w + h)
    return (rng.integers(0, 256, (3, h, w, 4), dtype=np.int64).astype(np.uint8),
            rng.integers(0, 256, (3, h, w, 4), dtype=np.int64).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def batch(name):
    """(A, B) of a named batch: 'constant', 'constant_rgb', 'periodic_30x28', 'periodic_139x75', 'letterbox', 'pillarbox',
    'tile_74x42', ...; cached, read-only."""
    if name in ("constant", "constant_rgb"):
        A, B = constant_pairs(per_channel=name == "constant_rgb")
    elif name.startswith("periodic_"):
        w, h = (int(v) for v in name[len("periodic_"):].split("x"))
        _, A, B = periodic_pairs(w, h)
    elif name in ("letterbox", "pillarbox"):
        A, B = next((a, b) for n, a, b in letterbox_pairs() if n == name)
    elif name.startswith("tile_"):
        w, h = (int(v) for v in name[len("tile_"):].split("x"))
        A, B = tile_edge_triple(w, h)
    else:
        raise ValueError(name)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


BATCHES = (["constant", "constant_rgb"] + [f"periodic_{w}x{h}" for w, h in PERIODIC_SIZES] + ["letterbox", "pillarbox"]
           + [f"tile_{w}x{h}" for w, h in TILE_EDGE_SHAPES])


@functools.lru_cache(maxsize=None)
def witness(name):
    """float64 SSIM (the definition) of every pair of the batch: (N,) float64, computed once."""
    A, B = batch(name)
    out = np.array([M64.ssim(a, b) for a, b in zip(A, B)])
    out.setflags(write=False)
    return out
