"""Float64 yardstick for the dense-flow warp + blend (warp_blend_pixel in nus_warp_device.hpp and every kernel built on it).

The contract, derived from the kernel's arithmetic, not measured on it.  Inputs: frames A and B (u8), the
times t and nt = 1 - t as the f32 values the kernel uses (nt is the f32 difference), the flow as the f32 values the kernel sees
(an f16 field widened exactly).  Everything below is float64.

  positions   A is sampled at p - t f, B at p + nt f.  The product of two f32 values is exact in float64 (48 bits); its sum with
              the pixel index is exact too whenever the flow has no bits below 2^-40 (f16 fields, block vectors, dyadic flows), and
              otherwise carries a relative error of 2^-53, ten orders of magnitude below the band.
  clamp       each coordinate to [0, w - 1] / [0, h - 1].
  value       s = bilinear value with x0 = floor(x), x1 = min(x0 + 1, w - 1), likewise in y: the reference's geometry
              (warp_samples64).  The kernel's corner form (texel pair from min(x0, w - 2), fraction against that corner) must give
              the same value.
  candidates  floor(s) always; floor(s) - 1 if s - floor(s) <= eps; floor(s) + 1 if floor(s) + 1 - s <= eps; all inside [0, 255].
              Where nothing is rounded, floor(s) is the only candidate.  That is so where the f32 position is exact (ex = ey = 0
              below) and both fractions are multiples of 2^-8: then 1 - xf is exact, a texel times a fraction has at most 16
              significant bits, a horizontal lerp is a multiple of 2^-8 below 256, and its product with a vertical fraction and
              the vertical sum are multiples of 2^-16 below 256 -- 24 bits, exact in f32 in either form.  Positions that are
              integers on both axes (zero flow, clamped far-outside vectors, whole-pixel motion: the sample is a texel) are the
              plainest case; integer block vectors at times k / 8 are another.
  byte        trunc(f32(nt sa) + f32(t sb)), the CPU's three f32 roundings in both modes (the header comment of warp_blend_pixel
              says why), evaluated in numpy float32, for some candidate pair (sa, sb).  A sample is *decided* when both of its
              samples have one candidate: its byte is then fully determined.

The band: eps = 255 (ex + ey) + 2^-14.
  ex, ey      the worst error of the f32 position on each axis, after the clamp.
              position_ulps = 1/2 (FMA mode: the position is ONE correctly rounded FMA): 1/2 ulp32 of the coordinate.
              position_ulps = 1 (the oracle, EXACT mode: product and sum rounded separately): 1/2 ulp32 of the product t f plus 1/2
              ulp32 of the coordinate -- at most 1 ulp32 of the coordinate whenever |t f| <= |x|, and still a bound when a large
              vector lands near the left or top border.
              A rounding of an exactly representable value contributes nothing; and a real position at or beyond a border clamps
              to that border exactly in either form (rounding is monotone, 0 and w - 1 are representable, so is the pixel index
              the product is compared with), so there ex = 0.
  255         bounds the slope of a bilinear surface over u8 texels along either axis, and the surface is continuous across texel
              boundaries, so the value at the f32 position is within 255 (ex + ey) of s.
  2^-14       bounds the arithmetic of the three lerps at magnitude <= 255, given the f32 position.  The fraction x - corner is
              exact in f32; 1 - xf is one rounding, <= 2^-25, worth <= 255 * 2^-25 = 7.6e-6 per lerp.  FMA form, fma(b, f, a nf):
              one rounded product and one rounded FMA, each <= 1/2 ulp(255) = 2^-17, so <= 2.3e-5 per lerp.  The vertical lerp
              averages the errors of top and bottom (weights nyf + yf = 1) and adds its own: <= 4.6e-5.  Separately rounded form,
              a nf + b f: three roundings per lerp, 2 (3 * 2^-17 + 255 * 2^-25) = 0.999 * 2^-14.  Both are under 2^-14 = 6.1e-5.

The contract rejects what "within 1 LSB of the oracle, fewer than 0.1 % different" lets through (tests/test_warp64_contract.py): a
biased position, rounding instead of truncation, a handful of samples one count high, the wrong border fraction, swapped times,
a fused blend, a negated flow component, swapped channels.  Pure numpy, banded by rows so a 1920-wide strip stays small; no import
of the product's tables or of the oracle's warp."""
import numpy as np

ARITH_BAND = 2.0 ** -14
_BAND_PIXELS = 1 << 15  # pixels per row band: a few MiB of float64 per temporary


def _ulp32(v):
    """The spacing of f32 in the binade of |v| (float64 in, float64 out); 0 at 0."""
    v = np.abs(v)
    _, e = np.frexp(v)  # v in [2^(e-1), 2^e)
    return np.where(v == 0.0, 0.0, np.ldexp(1.0, np.maximum(e, -125) - 24))


def _is_f32(v):
    return v == v.astype(np.float32).astype(np.float64)


def _axis(p, coef, f, n, position_ulps):
    """The clamped real position p + coef f on an axis of n texels and the worst error of its f32 evaluation after the clamp."""
    prod = coef * f
    x = p + prod
    e1 = (position_ulps - 0.5) * _ulp32(prod) * ~_is_f32(prod)  # the separately rounded product, if the form has one
    e2 = 0.5 * _ulp32(np.abs(x) + e1) * (~_is_f32(x) | (e1 > 0.0))  # the rounding of the sum (of the FMA)
    outside = (x <= 0.0) | (x >= n - 1.0)
    return np.clip(x, 0.0, n - 1.0), np.where(outside, 0.0, e1 + e2)


def warp_samples64(img, x, y):
    """The clamp-to-edge bilinear samples of one (h, w, 4) uint8 frame at positions (x, y) (float64 arrays of one shape), in
    float64 and NOT truncated: shape x.shape + (4,).  x0 = floor(x), x1 = min(x0 + 1, w - 1), likewise in y."""
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] == 4 and img.dtype == np.uint8, (img.shape, img.dtype)
    h, w = img.shape[:2]
    x = np.clip(np.asarray(x, np.float64), 0.0, w - 1.0)
    y = np.clip(np.asarray(y, np.float64), 0.0, h - 1.0)
    xfl, yfl = np.floor(x), np.floor(y)
    x0, y0 = xfl.astype(np.int64), yfl.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    xf, yf = (x - xfl)[..., None], (y - yfl)[..., None]
    px = img.astype(np.float64)
    top = px[y0, x0] * (1.0 - xf) + px[y0, x1] * xf
    bottom = px[y1, x0] * (1.0 - xf) + px[y1, x1] * xf
    return top * (1.0 - yf) + bottom * yf


def _candidates(img, p_x, p_y, coef, flow, position_ulps):
    """One frame's samples at p + coef flow over a row band: s, floor(s), and whether floor(s) - 1 / floor(s) + 1 are allowed."""
    h, w = img.shape[:2]
    x, ex = _axis(p_x, coef, flow[..., 0], w, position_ulps)
    y, ey = _axis(p_y, coef, flow[..., 1], h, position_ulps)
    s = warp_samples64(img, x, y)
    eps = (255.0 * (ex + ey) + ARITH_BAND)[..., None]
    # nothing to round (see the module docstring): exact position, fractions on the 2^-8 grid -- texels among them
    exact = ((ex == 0.0) & (ey == 0.0) & (x * 256.0 == np.floor(x * 256.0)) & (y * 256.0 == np.floor(y * 256.0)))[..., None]
    lo = np.floor(s)
    below = ~exact & (s - lo <= eps) & (lo >= 1.0)
    above = ~exact & (lo + 1.0 - s <= eps) & (lo <= 254.0)
    return s, lo, below, above


def _blend32(sa, sb, t32, nt32):
    """trunc(f32(nt sa) + f32(t sb)): every product and the sum rounded to f32."""
    return np.floor(nt32 * sa.astype(np.float32) + t32 * sb.astype(np.float32))


def edge_flow(n, w, h, t, seed, kind="gauss", sigma=6.0):
    """Test content: n f32 flow fields (n, h, w, 2) that reach every branch of the sample for time t.  The body is Gaussian of
    `sigma` px ("gauss") or smooth waves of that amplitude ("smooth"); on top of it, where the frame has the rows: far-outside
    vectors in two corners, row 1 zero, row 2 whole-pixel (even vectors), row 3 vectors that put the A sample into
    [w - 2, w - 1] x [h - 2, h - 1] and row 4 the B sample, the first pixels of both at exactly (w - 1, h - 1) when t is dyadic."""
    rng = np.random.default_rng(seed + 7919 * w + 31 * h)
    t32 = np.float32(t)
    nt32 = np.float32(1.0) - t32
    if kind == "smooth":
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        flow = np.empty((n, h, w, 2), np.float32)
        for i in range(n):
            p, f = rng.uniform(0, 2 * np.pi, 4), rng.uniform(17, 61, 4)
            flow[i, ..., 0] = sigma * np.sin(x / f[0] + p[0]) * np.cos(y / f[1] + p[1])
            flow[i, ..., 1] = sigma * np.cos(x / f[2] + p[2]) * np.sin(y / f[3] + p[3])
    else:
        flow = (rng.standard_normal((n, h, w, 2)) * sigma).astype(np.float32)
    flow[:, 0, 0] = (1000.0, -1000.0)
    flow[:, -1, -1] = (-1000.0, 1000.0)
    if h >= 5 and w >= 8:
        flow[:, 1] = 0.0
        flow[:, 2] = rng.integers(-3, 4, (n, w, 2)) * 2.0
        px, py = np.arange(w, dtype=np.float64), np.array([3.0, 4.0])
        for row, coef in ((3, -float(t32)), (4, float(nt32))):  # p + coef f = target
            if coef == 0.0:
                continue
            u = rng.uniform(0.0, 1.0, (n, w, 2))
            u[:, :4] = 1.0
            flow[:, row, :, 0] = (w - 2 + u[..., 0] - px) / coef
            flow[:, row, :, 1] = (h - 2 + u[..., 1] - py[row - 3]) / coef
    return flow


def warp_contract(got, a, b, flow, t, position_ulps, tag, raise_on_violation=True, channels=(0, 1, 2, 3)):
    """Hold uint8 `got` to the contract above.  One pair: a, b (h, w, 4), flow (h, w, 2) f32 or f16 (None: zero flow), and got
    (h, w, 4) for a scalar t or (K, h, w, 4) for a list of K times.  A stack of n pairs: a, b (n, h, w, 4), flow (n, h, w, 2), got
    (n, h, w, 4) or (n, K, h, w, 4).  position_ulps: 0.5 for FMA mode, 1 for the separately rounded form.
    Returns {"samples", "decided", "differ_from_floor", "violations"}; raises AssertionError naming the first offenders -- (frame,
    time, y, x, channel), s of both samples, got -- unless raise_on_violation is False.  channels: the channels held and counted
    (an X input format defines its output alpha as 255 instead of blending it: the caller asserts that and holds 0, 1, 2)."""
    a, b, got = np.asarray(a), np.asarray(b), np.asarray(got)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and got.dtype == np.uint8 and a.shape == b.shape, (a.shape, b.shape, got.dtype)
    stack, multi = a.ndim == 4, np.ndim(t) > 0
    times = [np.float32(v) for v in (t if multi else [t])]
    if not stack:
        a, b, got = a[None], b[None], got[None]
        flow = None if flow is None else np.asarray(flow)[None]
    if not multi:
        got = got[:, None]
    n, h, w = a.shape[:3]
    assert got.shape == (n, len(times), h, w, 4), (got.shape, (n, len(times), h, w, 4))
    if flow is None:
        flow = np.zeros((n, h, w, 2), np.float32)
    flow = np.asarray(flow)
    assert flow.shape == (n, h, w, 2) and flow.dtype in (np.float32, np.float16), (flow.shape, flow.dtype)
    rows = max(1, _BAND_PIXELS // w)
    p_x = np.arange(w, dtype=np.float64)[None, :]
    ch = list(channels)
    held = got.size // 4 * len(ch)
    decided = differ = violations = 0
    first = []
    for i in range(n):
        for y_lo in range(0, h, rows):
            y_hi = min(h, y_lo + rows)
            fl = flow[i, y_lo:y_hi].astype(np.float64)
            p_y = np.arange(y_lo, y_hi, dtype=np.float64)[:, None]
            for k, t32 in enumerate(times):
                nt32 = np.float32(1.0) - t32
                s_a, lo_a, below_a, above_a = (v[..., ch] for v in _candidates(a[i], p_x, p_y, -float(t32), fl, position_ulps))
                s_b, lo_b, below_b, above_b = (v[..., ch] for v in _candidates(b[i], p_x, p_y, float(nt32), fl, position_ulps))
                g = got[i, k, y_lo:y_hi][..., ch].astype(np.float32)
                ok = g == _blend32(lo_a, lo_b, t32, nt32)
                differ += int((~ok).sum())
                for d_a, m_a in ((0.0, None), (-1.0, below_a), (1.0, above_a)):
                    for d_b, m_b in ((0.0, None), (-1.0, below_b), (1.0, above_b)):
                        if m_a is None and m_b is None:
                            continue
                        m = m_b if m_a is None else m_a if m_b is None else m_a & m_b
                        if m.any():
                            ok |= m & (g == _blend32(lo_a + d_a, lo_b + d_b, t32, nt32))
                decided += int((~(below_a | above_a | below_b | above_b)).sum())
                if not ok.all():
                    violations += int((~ok).sum())
                    for y, x, c in np.argwhere(~ok)[:max(0, 6 - len(first))]:
                        first.append(((i, k, int(y) + y_lo, int(x), ch[c]), float(s_a[y, x, c]), float(s_b[y, x, c]),
                                      int(got[i, k, y + y_lo, x, ch[c]])))
    st = {"samples": int(held), "decided": decided, "differ_from_floor": differ, "violations": violations}
    if violations and raise_on_violation:
        raise AssertionError(
            f"warp contract violated ({tag}): {violations} of {held} bytes are trunc(f32(nt sa) + f32(t sb)) for no candidate "
            f"pair (position_ulps = {position_ulps}); first (frame, time, y, x, channel), s of the A sample, s of the B sample, "
            f"got: {first}; decided share {decided / held:.4f}, {differ} bytes differ from the all-floor result")
    return st
