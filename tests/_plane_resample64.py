"""Float64 witness for the planar up-scaler of I420 frames (nus_yuv_resizer of include/nuscaler_hip.h).

`axis(in_n, out_n, filt, phi)` restates the header's axis geometry in numpy float32, expression by expression: a sample of index
i sits at i + phi on both sides of the axis (phi = 0.5: the crate's half-pixel convention; 0.25: 4:2:0 chroma co-sited with the
even luma column).  `sin` is evaluated in float64 and rounded, so a weight may differ from libm's sinf in the last bit.

`plane_resample64` resamples one 8-bit plane in float64, vertical pass then horizontal.  The vertical pass always takes
oracle.resize_axis' weights (phi = 0.5), and so does the horizontal pass at phi = 0.5: the centre case stays independent of the
product and of this file.  Only the horizontal pass at phi = 0.25 takes the restatement's weights.  The contract is
_resample64.assert_fma_contract with _resample64.eps_rule(Tx, Ty), unchanged."""
import numpy as np

F = np.float32
_SUPPORT = {0: F(3.0), 1: F(2.0), 2: F(1.0)}  # oracle.FILTER_LANCZOS3 / _CATMULLROM / _TRIANGLE
_PI = F(3.14159265358979323846)
MAX_TAPS = 32


def _sinc(t):
    a = F(t * _PI)
    if t == 0:
        return F(1.0)
    return F(F(np.sin(np.float64(a))) / a)


def _kernel(filt, x):
    x = F(x)
    a = F(abs(x))
    if filt == 0:
        return F(_sinc(x) * _sinc(F(x / F(3.0)))) if a < F(3.0) else F(0.0)
    if filt == 1:  # the crate's bicubic_kernel(x, b = 0, c = 0.5)
        a2 = F(a * a)
        a3 = F(a2 * a)
        if a < F(1.0):
            k = F(F(F(F(9.0) * a3) + F(F(-15.0) * a2)) + F(6.0))
        elif a < F(2.0):
            k = F(F(F(F(F(-3.0) * a3) + F(F(15.0) * a2)) + F(F(-24.0) * a)) + F(12.0))
        else:
            k = F(0.0)
        return F(k / F(6.0))
    return F(F(1.0) - a) if a < F(1.0) else F(0.0)


def axis(in_n, out_n, filt, phi):
    """(left int64 [out_n], ntaps int64 [out_n], weights float32 [out_n, MAX_TAPS]) of the axis in_n -> out_n with sample
    position phi, in the header's expression order."""
    phi = F(phi)
    support = _SUPPORT[filt]
    ratio = F(F(in_n) / F(out_n))
    sratio = ratio if ratio >= F(1.0) else F(1.0)
    src_support = F(support * sratio)
    left = np.zeros(out_n, np.int64)
    ntaps = np.zeros(out_n, np.int64)
    w = np.zeros((out_n, MAX_TAPS), np.float32)
    for o in range(out_n):
        centre = F(F(F(o) + phi) * ratio)
        if phi != F(0.5):
            centre = F(centre + F(F(0.5) - phi))
        lo = int(np.floor(F(centre - src_support)))
        lo = min(max(lo, 0), in_n - 1)
        hi = int(np.ceil(F(centre + src_support)))
        hi = min(max(hi, lo + 1), in_n)
        centre = F(centre - F(0.5))
        n = hi - lo
        assert n <= MAX_TAPS
        ws = [_kernel(filt, F(F(F(lo + i) - centre) / sratio)) for i in range(n)]
        s = F(0.0)
        for x in ws:
            s = F(s + x)
        left[o], ntaps[o] = lo, n
        w[o, :n] = [F(x / s) for x in ws]
    return left, ntaps, w


def windows(in_n, out_n, filt, phi):
    """(left int64 [k, max out_n], ntaps int64 [k, max out_n], valid bool [k, max out_n]) of the axes in_n -> out_n[0..k), all at
    once: the window expressions of `axis` in the same float32 order (a window needs no weight, so no libm either).  Slots at
    o >= out_n[i] are not valid and hold 0."""
    out_n = np.atleast_1d(np.asarray(out_n, np.int64))
    phi = F(phi)
    ratio = (F(in_n) / out_n.astype(F))[:, None]
    src_support = _SUPPORT[filt] * np.maximum(ratio, F(1.0))
    o = np.arange(int(out_n.max()), dtype=np.int64)[None, :]
    centre = (o.astype(F) + phi) * ratio
    if phi != F(0.5):
        centre = centre + F(F(0.5) - phi)
    assert centre.dtype == F and src_support.dtype == F
    lo = np.clip(np.floor(centre - src_support).astype(np.int64), 0, in_n - 1)
    hi = np.minimum(np.maximum(np.ceil(centre + src_support).astype(np.int64), lo + 1), in_n)
    valid = o < out_n[:, None]
    return np.where(valid, lo, 0), np.where(valid, hi - lo, 0), valid


def row_geometry(left, ntaps, out_n, run=4, segment=256):
    """(ncols_max, union) of an x axis in the row kernel, by the two loops of YuvResizer::initialize: the widest dword-aligned input
    footprint of a segment of 256 outputs, and the widest union of the windows of a lane's run of 4 outputs."""
    assert out_n % run == 0
    left, end = np.asarray(left, np.int64)[:out_n], np.asarray(left, np.int64)[:out_n] + np.asarray(ntaps, np.int64)[:out_n]
    ncols = 0
    for x0 in range(0, out_n, segment):
        xl = min(x0 + segment, out_n) - 1
        ncols = max(ncols, (int(end[xl]) - (int(left[x0]) & ~3) + 3) & ~3)
    union = int((end.reshape(-1, run).max(axis=1) - left[::run]).max())
    return ncols, union


def _oracle_axis(oracle_mod, in_n, out_n, filt):
    left, ntaps, w = oracle_mod.resize_axis(in_n, out_n, filt)
    return left.astype(np.int64), ntaps.astype(np.int64), np.asarray(w, np.float32)


def plane_axes(oracle_mod, iw, ih, ow, oh, filt, phi_x):
    """((left, ntaps, weights) of x, of y) as plane_resample64 uses them."""
    ax = _oracle_axis(oracle_mod, iw, ow, filt) if float(phi_x) == 0.5 else axis(iw, ow, filt, phi_x)
    return ax, _oracle_axis(oracle_mod, ih, oh, filt)


def plane_eps(oracle_mod, iw, ih, ow, oh, filt, phi_x):
    from _resample64 import eps_rule

    (_, nx, _), (_, ny, _) = plane_axes(oracle_mod, iw, ih, ow, oh, filt, phi_x)
    return eps_rule(int(nx.max()), int(ny.max()))


def plane_resample64(oracle_mod, plane, ow, oh, filt, phi_x=0.5):
    """One (h, w) uint8 plane -> (oh, ow) float64: vertical pass, then horizontal.  Equal sizes: a copy, as imageops::resize."""
    plane = np.asarray(plane)
    assert plane.ndim == 2 and plane.dtype == np.uint8, plane.shape
    ih, iw = plane.shape
    if (iw, ih) == (ow, oh):
        return plane.astype(np.float64)
    (lx, nx, wx), (ly, ny, wy) = plane_axes(oracle_mod, iw, ih, ow, oh, filt, phi_x)
    src = plane.astype(np.float64)
    tmp = np.zeros((oh, iw), np.float64)
    for i in range(int(ny.max())):  # (slots beyond a window's taps hold weight 0; their clipped index reads a real row)
        tmp += wy[:, i, None].astype(np.float64) * src[np.minimum(ly + i, ih - 1)]
    out = np.zeros((oh, ow), np.float64)
    for j in range(int(nx.max())):
        out += wx[None, :, j].astype(np.float64) * tmp[:, np.minimum(lx + j, iw - 1)]
    return out
