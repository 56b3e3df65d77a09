"""Float64 witness of the two FSR1-style shaders (nu_scaler_core/src/upscale/fsr.rs:24-166 EASU, :171-259 RCAS), written from
their definitions: vectorised numpy float64, no helper shared with oracle/oracle_np.py (an f32 twin of the C oracle), no import of
the product.  It holds the C oracle (tests/test_fsr64_contract.py) and the HIP kernels, EXACT and FAST
(tests/test_gpu_fsr_witness.py).

What a witness returns, per colour sample (h, w, 3): `v` = 255 clamp(colour, 0, 1) in float64, a half-width `eps`, a mask
`decided`, and `pinned` (a byte, or -1).  The contract (fsr_contract): a decided sample's byte lies in
[floor(v - eps), floor(v + eps)], cut to [0, 255]; where pinned >= 0 it IS that byte; alpha is 255 (fsr.rs:165, :258).

Everything below counts f32 roundings.  U = 2^-24: a correctly rounded f32 operation with a result below 1 errs by at most U / 2,
below 2 by U, below 4 by 2 U, ...; hu(x) is that half ulp for the magnitude of x.  The constants 0.0001, 0.299, 0.587, 0.114, 0.2
and the sharpness values are the f32 constants of the shader, widened.

EASU (fsr.rs:104-166)
  geometry    inCoord c = (g + 0.5) * (in / out) (fsr.rs:110-114).  Float64: (g + 0.5) * in is exact, one division.  f32: g + 0.5 is
              exact, the scale and the product are one rounding each, so |c32 - c| <= 2 U c (1 + 2^-20); fract(c) = c - floor(c)
              (fsr.rs:118) is exact in f32 given c32.  So dfx = 2 U cx (1 + 2^-20), likewise dfy -- WHERE both integer parts agree;
              where they do not (the exact c is an integer or within 2 U c of one) the sample is undecided.
  dwx         FsrDirA (fsr.rs:87-101) and wx (fsr.rs:132).  A texel channel t / 255: U / 2.  A channel difference: two of those and
              its own rounding, 3 U / 2; |.| is exact.  The sum of three: 9 U / 2 carried, U for the first add (< 2), 2 U for the
              second (< 4): 15 U / 2.  Divided by 3: 5 U / 2 and U / 2 more.  Plus 0.0001: at most U (the sum may reach 1).  So
              dx = vgx + 0.0001 and dy carry a <= 4 U each.  normalize divides both by ONE length: its error cancels in
              wx = |dirx| / (|dirx| + |diry|), which is dx / (dx + dy) with four roundings left (the two quotients by the length, the
              sum, the last quotient), each <= U relative, on a value <= 1: 4 U.  d wx / d dx = dy / (dx + dy)^2 and
              d wx / d dy = -dx / (dx + dy)^2, so the carried part is <= a / (dx + dy).  dwx = 4 U / (dx + dy) + 4 U.
              wy = 1 - wx (fsr.rs:133): dwx and U / 2.
  tap i       offsets px = x - fx, py = y - fy (fsr.rs:142): dfx + hu(px), dfy + hu(py).  dist = |px wx + py wy| (fsr.rs:145) with
              wy = 1 - wx moves by (px - py) per unit of wx:
                dd_i = |px - py| dwx + |py| U / 2 + wx (dfx + hu(px)) + wy (dfy + hu(py)) + hu(px wx) + hu(py wy) + hu(d).
              FsrCubic (fsr.rs:74-84) is continuous at d = 1 (both pieces give 1) and JUMPS from 1 to 0 at d = 2: a sample with
              any tap at |d_i - 2| <= dd_i is undecided, whatever its value.  Tap (1, 1) always has d <= 1 and the weights on
              d <= 2 lie in [1, 2], so the weight sum is >= 1 and max(sumWeight, 0.0001) (fsr.rs:155) never binds.
  weight i    |w'| is |-1.5 - 1.5 d^2 + 2 d| on d <= 1 and |-0.5 + 5 d - 3 d^2| on 1 < d <= 2 (the larger of the two where
              |d - 1| <= dd_i), and |w''| <= 7 (|5 - 6 d| at d = 2), so the distance error moves the weight by at most
              (|w'(d_i)| + 7 dd_i) dd_i.  Evaluating the polynomial in f32, results below 1 erring by U / 2, below 2 by
              U and so on: d <= 1 -- d2 (U / 2), d3 (U / 2 carried, U / 2), 1.5 d (U), 2 - 1.5 d (U carried, U), - 0.5 d3 (U / 2
              carried, U), + d2 (U / 2 carried, U; the result lies in [1, 2]): rho = 5 U.  1 < d <= 2 -- d2 < 4 (2 U), d3 < 8 (4 U
              carried, 4 U), 2.5 d2 <= 10 (5 U carried, 8 U), - 0.5 d + 2.5 d2 <= 9 (13 U carried, 8 U), - d3 (8 U carried, U; the
              result lies in [1, 1.51]): rho = 30 U.
              werr_i = rho_i + (|w'(d_i)| + 7 dd_i) dd_i.
  colour      sum c_i w_i / sum w_i (fsr.rs:149-155) moves by sum |c_i - colour| werr_i / (sum w - sum werr) for the weights, and
              by K U for its own arithmetic, colour <= 1: 16 products and 15 adds on partial sums <= the weight sum (16 U relative
              to it), 15 adds of the weight sum (15 U), the quotient (U / 2), the taps' own unpack (U / 2), mix (fsr.rs:160:
              1 - s, two products, one sum: 2 U, and the centre's unpack U / 2), the product with 255 (2^-17 at 255 = 255 U / 2):
              K = 35.  The weight term shrinks by 1 - s under the mix.
  eps = 255 (35 U + (1 - s) sum_i |c_i - colour| werr_i / (sum w - sum werr)).

FAST (option fsr_fast: FsrCubic from a table of 128 cells per unit of d with linear interpolation, FMA sums, reciprocal and one
Newton step; distances, piece decisions and the direction weight as above).  From the definition, not from the kernel:
  table       linear interpolation with h = 1 / 128 errs by h^2 / 8 max |f''|: |2 - 3 d| <= 2 on d <= 1, |5 - 6 d| <= 7 on
              1 < d <= 2: 2 / (8 * 128^2) = 1.53e-5 and 7 / (8 * 128^2) = 5.34e-5 per weight.  The entries are f32 evaluations
              of the polynomial at the cell's ends (rho above, a convex combination of two of them), the stored difference is one
              rounding more and the interpolating FMA another: 2 U.  werr_i grows by lut_i + 2 U.
  quotient    a reciprocal good to 1 ulp, refined by z (2 - den z): one FMA and one product, 2 U relative, and z's remaining error
              squared (2^-46); the product with the sum: U.  3.5 U where the division had U / 2: K = 38.  The FMA sums round less
              often than the separate products and adds counted in K.

RCAS (fsr.rs:218-258): no discontinuity, every sample is decided.
  luma        three products and two adds below 1 (5 U / 2) and the unpack of three channels, weights summing to 1 (U / 2): 3 U.
  contrast    max - min: 6 U and U / 2.  Divided by 0.2: 32.5 U and U / 2: dst = 33 U.
  smoothstep  t = clamp(st, 0, 1), t t (3 - 2 t): slope 6 t (1 - t) <= 1.5, so 49.5 U carried; t t (U / 2, times 3), 3 - 2 t (2 U),
              the product (U / 2): 54 U with the rounding of 1 - smoothstep.  strength = s (1 - smoothstep): dstr = 54 U s + U / 2.
  laplacian   4 c - t - b - l - r: five unpacks (4 U / 2 + 4 U / 2) and four differences below 4 (2 U each): dlap = 12 U.
  result      c + lap strength: U / 2 + |lap| dstr + strength dlap + hu(lap strength) + hu(result); times 255: 2^-17.
  pinned      where the strength is exactly zero IN F32 -- sharpness 0, or st >= 1 + dst so that the clamp returns 1 and
              smoothstep 1 -- the shader computes c + lap * 0 = f32(C / 255), and the byte is u32(f32(C / 255) * 255): a 256-entry
              table, computed once in np.float32 from the definition of unpack and pack (fsr.rs:191-205).  It is C or C - 1.
              A zero laplacian with a non-zero strength is NOT pinned: 4 c - c - c - c - c is not exact in f32.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
K_EXACT, K_FAST = 35.0, 38.0
LUT_NEAR, LUT_FAR = 2.0 / (8.0 * 128.0 ** 2), 7.0 / (8.0 * 128.0 ** 2)
_C = {k: float(np.float32(k)) for k in (0.0001, 0.001, 0.299, 0.587, 0.114, 0.2)}

Witness = namedtuple("Witness", "v eps decided pinned")

# u32(f32(C / 255) * 255): unpack then the truncating pack (fsr.rs:191-205), in the shader's own f32
PACK_OF_UNPACK = (np.arange(256, dtype=np.float32) / np.float32(255.0) * np.float32(255.0)).astype(np.uint32).astype(np.int16)


def _hu(v):
    """Half an f32 ulp at the magnitude of v (the next binade's when v is within 2^-20 of it)."""
    _, e = np.frexp(np.abs(v) * (1.0 + 2.0 ** -20))
    return np.ldexp(1.0, np.maximum(e, -100) - 25)


def _rgb(img):
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] == 4 and img.dtype == np.uint8, (img.shape, img.dtype)
    return img[..., :3].astype(np.float64) / 255.0  # fsr.rs:46-53


def _axis(n_out, n_in):
    """inCoord on one axis (fsr.rs:110-118): integer part, fract, the f32 error of fract, and where f32 has the same integer part."""
    g = np.arange(n_out, dtype=np.float64)
    c = (g + 0.5) * n_in / n_out
    c32 = ((g.astype(np.float32) + np.float32(0.5)) * (np.float32(n_in) / np.float32(n_out))).astype(np.float64)
    i = np.floor(c)
    return i.astype(np.int64), c - i, 2.0 * U * c * (1.0 + 2.0 ** -20), np.floor(c32) == i


def easu64(img, ow, oh, sharp, fast=False):
    """EASU of one (h, w, 4) uint8 frame to ow x oh: Witness of (oh, ow, 3) arrays (decided: (oh, ow, 1))."""
    px = _rgb(img)
    ih, iw = px.shape[:2]
    ix, fx, dfx, same_x = _axis(ow, iw)
    iy, fy, dfy, same_y = _axis(oh, ih)
    fx, dfx, fy, dfy = fx[None, :], dfx[None, :], fy[:, None], dfy[:, None]

    def fetch(ox, oy):  # FsrEasuF, fsr.rs:64-71
        return px[np.clip(iy + oy, 0, ih - 1)[:, None], np.clip(ix + ox, 0, iw - 1)[None, :]]

    # FsrDirA, fsr.rs:87-101: "vgx" is the difference of the texels above and below
    vgx = np.abs(fetch(0, -1) - fetch(0, 1)).sum(-1) / 3.0
    vgy = np.abs(fetch(-1, 0) - fetch(1, 0)).sum(-1) / 3.0
    dx, dy = vgx + _C[0.0001], vgy + _C[0.0001]
    length = np.sqrt(dx * dx + dy * dy)
    dirx, diry = dx / length, dy / length
    wx = np.abs(dirx) / (np.abs(dirx) + np.abs(diry))  # fsr.rs:132-133
    wy = 1.0 - wx
    dwx = 4.0 * U / (dx + dy) + 4.0 * U

    def tap(x, y):
        po_x, po_y = x - fx, y - fy  # fsr.rs:142
        a, b = po_x * wx, po_y * wy
        d = np.abs(a + b)  # fsr.rs:145
        dd = (np.abs(po_x - po_y) * dwx + np.abs(po_y) * (U / 2) + wx * (dfx + _hu(po_x)) + wy * (dfy + _hu(po_y))
              + _hu(a) + _hu(b) + _hu(d))
        return d, dd

    def cubic(d):  # fsr.rs:74-84
        d2 = d * d
        d3 = d * d2
        return np.where(d <= 1.0, 2.0 - 1.5 * d - 0.5 * d3 + d2, np.where(d <= 2.0, 0.0 - 0.5 * d + 2.5 * d2 - d3, 0.0))

    num = np.zeros((oh, ow, 3))
    den = np.zeros((oh, ow))
    jump = np.zeros((oh, ow), bool)
    for y in range(4):
        for x in range(4):
            d, dd = tap(x, y)
            jump |= np.abs(d - 2.0) <= dd
            w = cubic(d)
            num += fetch(x - 1, y - 1) * w[..., None]  # fsr.rs:117, :127, :149-150
            den += w
    col = num / np.maximum(den, _C[0.0001])[..., None]  # fsr.rs:155

    err = np.zeros((oh, ow, 3))
    err_w = np.zeros((oh, ow))
    for y in range(4):
        for x in range(4):
            d, dd = tap(x, y)
            s_near, s_far = np.abs(-1.5 - 1.5 * d * d + 2.0 * d), np.abs(-0.5 + 5.0 * d - 3.0 * d * d)
            near, off = d <= 1.0 - dd, d > 2.0
            seam = ~near & (d <= 1.0 + dd)
            slope = np.where(near, s_near, np.where(seam, np.maximum(s_near, s_far), s_far))
            rho = np.where(near, 5.0 * U, 30.0 * U)
            if fast:
                rho = rho + np.where(near, LUT_NEAR, LUT_FAR) + 2.0 * U
            werr = np.where(off, 0.0, rho + (slope + 7.0 * dd) * dd)
            err += np.abs(fetch(x - 1, y - 1) - col) * werr[..., None]
            err_w += werr
    mixed = np.float32(sharp) > np.float32(0.001)  # fsr.rs:158
    s = float(np.float32(sharp)) if mixed else 0.0
    if mixed:
        col = col * (1.0 - s) + fetch(0, 0) * s  # mix, fsr.rs:159-160
    k = K_FAST if fast else K_EXACT
    eps = 255.0 * (k * U + (1.0 - s) * err / np.maximum(den - err_w, 0.5)[..., None])
    decided = (same_x[None, :] & same_y[:, None] & ~jump)[..., None]
    return Witness(255.0 * np.clip(col, 0.0, 1.0), eps, decided, np.full((oh, ow, 3), -1, np.int16))


def rcas64(img, sharp):
    """RCAS of one (h, w, 4) uint8 frame: Witness of (h, w, 3) arrays."""
    img = np.asarray(img)
    px = _rgb(img)
    h, w = px.shape[:2]
    gx, gy = np.arange(w), np.arange(h)

    def fetch(ox, oy):  # FsrRcasSample, fsr.rs:208-215
        return px[np.clip(gy + oy, 0, h - 1)[:, None], np.clip(gx + ox, 0, w - 1)[None, :]]

    c, t, b, l, r = fetch(0, 0), fetch(0, -1), fetch(0, 1), fetch(-1, 0), fetch(1, 0)  # fsr.rs:226-230
    lum = [p[..., 0] * _C[0.299] + p[..., 1] * _C[0.587] + p[..., 2] * _C[0.114] for p in (c, t, b, l, r)]  # fsr.rs:233-237
    contrast = np.maximum.reduce(lum) - np.minimum.reduce(lum)  # fsr.rs:240-244
    st = contrast / _C[0.2]
    tt = np.clip(st, 0.0, 1.0)  # smoothstep(0, 0.2, .), fsr.rs:247
    s = float(np.float32(sharp))
    strength = (s * (1.0 - tt * tt * (3.0 - 2.0 * tt)))[..., None]
    lap = 4.0 * c - t - b - l - r  # fsr.rs:251
    term = lap * strength
    res = c + term  # fsr.rs:254
    dstr = 54.0 * U * s + U / 2
    eps = 255.0 * (U / 2 + np.abs(lap) * dstr + strength * 12.0 * U + _hu(term) + _hu(res)) + 2.0 ** -17
    zero = np.broadcast_to(((st >= 1.0 + 33.0 * U) | (s == 0.0))[..., None], res.shape)
    pinned = np.where(zero, PACK_OF_UNPACK[img[..., :3]], np.int16(-1)).astype(np.int16)
    return Witness(255.0 * np.clip(res, 0.0, 1.0), eps, np.ones((h, w, 1), bool), pinned)


def permitted(wit):
    """The inclusive byte range [lo, hi] every sample of a Witness may take (int16 arrays)."""
    lo = np.clip(np.floor(wit.v - wit.eps), 0, 255).astype(np.int16)
    hi = np.clip(np.floor(wit.v + wit.eps), 0, 255).astype(np.int16)
    pin = wit.pinned >= 0
    return np.where(pin, wit.pinned, lo), np.where(pin, wit.pinned, hi)


def fsr_contract(got, wit, tag, raise_on_violation=True):
    """Hold uint8 `got` (h, w, 4) to a Witness.  Returns {"samples", "decided", "single", "differ_from_floor", "violations"}: colour
    samples, those decided, those decided with ONE permitted byte, decided ones that are not floor(v), and decided ones outside
    their range; raises AssertionError naming the first offenders -- (y, x, channel), v, eps, got -- unless told not to."""
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == wit.v.shape[:2] + (4,), (got.shape, got.dtype, wit.v.shape)
    assert (got[..., 3] == 255).all(), f"{tag}: alpha is not 255 everywhere"
    g = got[..., :3].astype(np.int16)
    lo, hi = permitted(wit)
    dec = np.broadcast_to(wit.decided, g.shape)
    bad = dec & ((g < lo) | (g > hi))
    floor_v = np.where(wit.pinned >= 0, wit.pinned, np.clip(np.floor(wit.v), 0, 255).astype(np.int16))
    st = {"samples": int(g.size), "decided": int(dec.sum()), "single": int((dec & (lo == hi)).sum()),
          "differ_from_floor": int((dec & (g != floor_v)).sum()), "violations": int(bad.sum())}
    if st["violations"] and raise_on_violation:
        first = [((int(y), int(x), int(c)), float(wit.v[y, x, c]), float(wit.eps[y, x, c]), int(g[y, x, c]))
                 for y, x, c in np.argwhere(bad)[:6]]
        raise AssertionError(f"FSR contract violated ({tag}): {st['violations']} of {st['decided']} decided samples lie outside "
                             f"[floor(v - eps), floor(v + eps)]; first (y, x, channel), v, eps, got: {first}; single-valued share "
                             f"{st['single'] / st['samples']:.4f}")
    return st


# The cases both test files run: the smallest sizes that reach each path of the launcher (tests/test_gpu_fsr_witness.py says
# which).  Exactly x1/2 is left out on purpose: fx = fy = 0 there, tap (2, 2) sits at d = 2 wx + 2 wy = 2 for EVERY sample and
# nothing is decided; at x3/2 that happens to one sample in nine.
CASES = [((32, 24), (64, 48)), ((17, 13), (40, 29)), ((100, 70), (257, 131)), ((5, 3), (130, 67)), ((64, 36), (96, 54)),
         ((70, 40), (64, 33)), ((20, 20), (20, 20)), ((1, 1), (3, 2))]
RCAS_CASE = (249, 17)  # RCAS alone: one 248-column strip and one column, one 16-row block and one row
EASU_SHARPNESS, RCAS_SHARPNESS = (0.0, 0.3), (0.7, 0.0)


def contents(oracle_mod, w, h):
    """The four test images of a size: noise, gradient, a flat 77 (v lands on an integer: two permitted bytes), and an edge image
    whose flat areas have equal gradients, wx = 0.5 exactly, so that taps sit at distance exactly 2."""
    flat = np.full((h, w, 4), 77, np.uint8)
    edge = np.zeros((h, w, 4), np.uint8)
    edge[:, w // 2:] = 200
    edge[h // 2:, :] //= 2
    return {"noise": oracle_mod.gen_noise(w, h, 77), "gradient": oracle_mod.gen_gradient(w, h), "flat": flat, "edge": edge}
