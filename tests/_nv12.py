"""Yardstick of the NV12 entry points ("NV12 frames" in include/nuscaler_hip.h): the layout, restated in numpy.  An NV12 frame is
the I420 frame's bytes in another place, so the expected bytes of every NV12 test are the I420 yardsticks' (tests/_yuv.py,
oracle.resize, tests/_plane_resample64.py) passed through `interleave`, or computed from `deinterleave` of the input."""
import numpy as np


def _layout(w, h, pitch=0, uv_offset=0):
    """(y_pitch, uv_pitch, effective uv_offset, frame bytes) as the header defines them."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if pitch == 0:
        assert uv_offset == 0
        return w, 2 * cw, w * h, w * h + 2 * cw * ch
    assert pitch >= 2 * cw and (uv_offset == 0 or uv_offset >= pitch * h)
    off = uv_offset or pitch * h
    return pitch, pitch, off, off + pitch * ch


def interleave(i420, w, h, pitch=0, uv_offset=0, fill=0):
    """One tight I420 frame (uint8 vector) -> the NV12 frame of that layout; every byte outside the rows holds `fill`."""
    i420 = np.asarray(i420, np.uint8).reshape(-1)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert i420.size == w * h + 2 * cw * ch
    yp, up, off, n = _layout(w, h, pitch, uv_offset)
    out = np.full(n, fill, np.uint8)
    y, u, v = i420[:w * h].reshape(h, w), i420[w * h:w * h + cw * ch].reshape(ch, cw), i420[w * h + cw * ch:].reshape(ch, cw)
    for r in range(h):
        out[r * yp:r * yp + w] = y[r]
    for r in range(ch):
        out[off + r * up:off + r * up + 2 * cw:2] = u[r]
        out[off + r * up + 1:off + r * up + 2 * cw:2] = v[r]
    return out


def deinterleave(nv12, w, h, pitch=0, uv_offset=0):
    """One NV12 frame of that layout -> the tight I420 frame."""
    nv12 = np.asarray(nv12, np.uint8).reshape(-1)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    yp, up, off, n = _layout(w, h, pitch, uv_offset)
    assert nv12.size >= off + up * (ch - 1) + 2 * cw
    y = np.stack([nv12[r * yp:r * yp + w] for r in range(h)])
    uv = np.stack([nv12[off + r * up:off + r * up + 2 * cw] for r in range(ch)])
    return np.concatenate([y.reshape(-1), uv[:, 0::2].reshape(-1), uv[:, 1::2].reshape(-1)])
