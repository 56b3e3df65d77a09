"""8-bit YUV 4:2:0 frames (I420 and NV12) <-> RGBA8 on the HIP device, bound to `nus_yuv*` / `nus_nv12*` of include/nuscaler_hip.h
(the integer contract is written there).  Build-defined: the reference has no YUV.  An I420 frame of w x h is its Y plane (w*h
bytes), then the U and V planes ((w+1)//2 * (h+1)//2 bytes each), rows tight.  An NV12 frame is its Y plane and one plane of
interleaved U,V byte pairs, the rows of both a pitch apart (`Nv12Layout`; tight by default): the I420 frame's bytes in another
place.  No torch type crosses into this module: the device entry points take integer device addresses, as
`SceneDetector.detect_device` does."""
from __future__ import annotations

import ctypes

from . import _capi as C
from .scene import _check, pixel_format
from .upscaler import _as_buffer

_MATRIX = {"bt601": C.YUV_MATRIX_BT601, "bt709": C.YUV_MATRIX_BT709}
_RANGE = {"limited": C.YUV_RANGE_LIMITED, "full": C.YUV_RANGE_FULL}
_SITING = {"center": C.YUV_SITING_CENTER, "left": C.YUV_SITING_LEFT}
_CHROMA = {"nearest": C.YUV_CHROMA_NEAREST, "bilinear": C.YUV_CHROMA_BILINEAR}


class _Format(ctypes.Structure):  # nus_yuv_format
    _fields_ = [("matrix", ctypes.c_int), ("range", ctypes.c_int), ("siting", ctypes.c_int), ("chroma_filter", ctypes.c_int)]


def _enum(name: str, table: dict, value) -> int:
    if isinstance(value, str):
        v = table.get(value.lower())
        if v is None:
            raise ValueError(f"{name} must be one of {', '.join(repr(k) for k in table)}, got {value!r}")
        return v
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"{name} must be one of {', '.join(repr(k) for k in table)}, got {value!r}")
    return value  # (an integer goes to the library as it is: the library refuses what it does not know)


class YuvFormat:
    """How the YUV side of a conversion is read or written: matrix "bt601" | "bt709", range "limited" | "full", siting "center"
    (Y4M 420jpeg) | "left" (420mpeg2), chroma "nearest" | "bilinear" (the up-sampling filter of to-RGBA; to-YUV always filters by
    the siting)."""

    def __init__(self, matrix="bt709", range="limited", siting="center", chroma="bilinear"):
        self.matrix = _enum("matrix", _MATRIX, matrix)
        self.range = _enum("range", _RANGE, range)
        self.siting = _enum("siting", _SITING, siting)
        self.chroma = _enum("chroma", _CHROMA, chroma)

    def _c(self) -> _Format:
        return _Format(self.matrix, self.range, self.siting, self.chroma)

    def __repr__(self):
        def name(table, v):
            return next((k for k, x in table.items() if x == v), v)

        return (f"YuvFormat(matrix={name(_MATRIX, self.matrix)!r}, range={name(_RANGE, self.range)!r}, "
                f"siting={name(_SITING, self.siting)!r}, chroma={name(_CHROMA, self.chroma)!r})")


def frame_bytes(w: int, h: int) -> int:
    """Bytes of one I420 frame (nus_yuv420_frame_bytes); ValueError for dimensions the library does not take."""
    n = int(C.lib().nus_yuv420_frame_bytes(int(w), int(h)))
    if n == 0:
        raise ValueError(C.last_error())
    return n


def coefficients(matrix="bt709", range="limited") -> tuple[list[int], list[int]]:
    """The Q14 tables the kernels use (nus_yuv_coefficients): (Yc, Uc, Vc over R, G, B; cy, rv, bu, gu, gv)."""
    a, b = (ctypes.c_int32 * 9)(), (ctypes.c_int32 * 5)()
    _check(C.lib().nus_yuv_coefficients(_enum("matrix", _MATRIX, matrix), _enum("range", _RANGE, range), ctypes.addressof(a),
                                        ctypes.addressof(b)))
    return list(a), list(b)


def to_rgba_device(d_yuv: int, w: int, h: int, d_rgba: int, fmt: YuvFormat | None = None, n_frames: int = 1, yuv_frame_stride: int = 0,
                   rgba_frame_stride: int = 0, rgba_format="rgba", stream: int = 0) -> None:
    """Enqueue I420 -> RGBA8 of `n_frames` device frames on `stream` (nus_yuv420_to_rgba8_device); strides in bytes, 0 = tight."""
    f = (fmt or YuvFormat())._c()
    _check(C.lib().nus_yuv420_to_rgba8_device(d_yuv or None, int(yuv_frame_stride), int(w), int(h), ctypes.addressof(f),
                                              pixel_format(rgba_format), d_rgba or None, int(rgba_frame_stride), int(n_frames),
                                              stream or None))


def to_yuv_device(d_rgba: int, w: int, h: int, d_yuv: int, fmt: YuvFormat | None = None, n_frames: int = 1, rgba_frame_stride: int = 0,
                  yuv_frame_stride: int = 0, rgba_format="rgba", stream: int = 0) -> None:
    """Enqueue RGBA8 -> I420 of `n_frames` device frames on `stream` (nus_rgba8_to_yuv420_device)."""
    f = (fmt or YuvFormat())._c()
    _check(C.lib().nus_rgba8_to_yuv420_device(d_rgba or None, int(rgba_frame_stride), int(w), int(h), ctypes.addressof(f),
                                              pixel_format(rgba_format), d_yuv or None, int(yuv_frame_stride), int(n_frames),
                                              stream or None))


def to_rgba(yuv_bytes, w: int, h: int, fmt: YuvFormat | None = None, rgba_format="rgba", device: int = 0) -> bytes:
    """One host I420 frame -> its RGBA8 pixels (nus_yuv420_to_rgba8)."""
    addr, n, keep = _as_buffer(yuv_bytes)
    out = bytearray(int(w) * int(h) * 4) if int(w) > 0 and int(h) > 0 else bytearray(4)
    o = (ctypes.c_ubyte * len(out)).from_buffer(out)
    f = (fmt or YuvFormat())._c()
    st = C.lib().nus_yuv420_to_rgba8(int(device), addr, n, int(w), int(h), ctypes.addressof(f), pixel_format(rgba_format),
                                     ctypes.addressof(o), len(out))
    del keep, o
    _check(st)
    return bytes(out)


def to_yuv(rgba_bytes, w: int, h: int, fmt: YuvFormat | None = None, rgba_format="rgba", device: int = 0) -> bytes:
    """One host RGBA8 frame -> its I420 frame (nus_rgba8_to_yuv420)."""
    addr, n, keep = _as_buffer(rgba_bytes)
    cap = int(w) * int(h) + 2 * ((int(w) + 1) // 2) * ((int(h) + 1) // 2) if int(w) > 0 and int(h) > 0 else 4
    out = bytearray(cap)
    o = (ctypes.c_ubyte * len(out)).from_buffer(out)
    f = (fmt or YuvFormat())._c()
    st = C.lib().nus_rgba8_to_yuv420(int(device), addr, n, int(w), int(h), ctypes.addressof(f), pixel_format(rgba_format),
                                     ctypes.addressof(o), len(out))
    del keep, o
    _check(st)
    return bytes(out)


class _Layout(ctypes.Structure):  # nus_nv12_layout
    _fields_ = [("pitch", ctypes.c_size_t), ("uv_offset", ctypes.c_size_t)]


class Nv12Layout:
    """Where the rows of an NV12 frame lie: `pitch` bytes between rows, of the Y plane and of the UV plane alike (0 = tight: w and
    2 * ((w + 1) // 2)); `uv_offset` bytes from the frame's base to its UV plane (0 = directly behind the Y rows).  The library
    refuses what the contract does not take (a pitch below the row, a uv_offset inside the Y plane)."""

    def __init__(self, pitch: int = 0, uv_offset: int = 0):
        for name, v in (("pitch", pitch), ("uv_offset", uv_offset)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
        self.pitch, self.uv_offset = pitch, uv_offset

    def _c(self) -> _Layout:
        return _Layout(self.pitch, self.uv_offset)

    def __repr__(self):
        return f"Nv12Layout(pitch={self.pitch}, uv_offset={self.uv_offset})"


def _layout(layout):
    """(the ctypes struct kept alive, its address or None) of an Nv12Layout or None (tight)."""
    if layout is None:
        return None, None
    if not isinstance(layout, Nv12Layout):
        raise ValueError(f"layout must be an Nv12Layout or None, got {layout!r}")
    c = layout._c()
    return c, ctypes.addressof(c)


def nv12_frame_bytes(w: int, h: int, layout: Nv12Layout | None = None) -> int:
    """Bytes of one NV12 frame (nus_nv12_frame_bytes); ValueError for dimensions or a layout the library does not take."""
    keep, addr = _layout(layout)
    n = int(C.lib().nus_nv12_frame_bytes(int(w), int(h), addr))
    del keep
    if n == 0:
        raise ValueError(C.last_error())
    return n


def nv12_to_rgba_device(d_nv12: int, w: int, h: int, d_rgba: int, fmt: YuvFormat | None = None, n_frames: int = 1, nv12_frame_stride: int = 0,
                        rgba_frame_stride: int = 0, rgba_format="rgba", stream: int = 0, layout: Nv12Layout | None = None) -> None:
    """Enqueue NV12 -> RGBA8 of `n_frames` device frames on `stream` (nus_nv12_to_rgba8_device); strides in bytes, 0 = tight."""
    f = (fmt or YuvFormat())._c()
    keep, la = _layout(layout)
    _check(C.lib().nus_nv12_to_rgba8_device(d_nv12 or None, la, int(nv12_frame_stride), int(w), int(h), ctypes.addressof(f),
                                            pixel_format(rgba_format), d_rgba or None, int(rgba_frame_stride), int(n_frames), stream or None))
    del keep


def rgba_to_nv12_device(d_rgba: int, w: int, h: int, d_nv12: int, fmt: YuvFormat | None = None, n_frames: int = 1, rgba_frame_stride: int = 0,
                        nv12_frame_stride: int = 0, rgba_format="rgba", stream: int = 0, layout: Nv12Layout | None = None) -> None:
    """Enqueue RGBA8 -> NV12 of `n_frames` device frames on `stream` (nus_rgba8_to_nv12_device)."""
    f = (fmt or YuvFormat())._c()
    keep, la = _layout(layout)
    _check(C.lib().nus_rgba8_to_nv12_device(d_rgba or None, int(rgba_frame_stride), int(w), int(h), ctypes.addressof(f),
                                            pixel_format(rgba_format), d_nv12 or None, la, int(nv12_frame_stride), int(n_frames), stream or None))
    del keep


def nv12_to_rgba(nv12_bytes, w: int, h: int, fmt: YuvFormat | None = None, rgba_format="rgba", device: int = 0) -> bytes:
    """One tight host NV12 frame -> its RGBA8 pixels (nus_nv12_to_rgba8)."""
    addr, n, keep = _as_buffer(nv12_bytes)
    out = bytearray(int(w) * int(h) * 4) if int(w) > 0 and int(h) > 0 else bytearray(4)
    o = (ctypes.c_ubyte * len(out)).from_buffer(out)
    f = (fmt or YuvFormat())._c()
    st = C.lib().nus_nv12_to_rgba8(int(device), addr, n, int(w), int(h), ctypes.addressof(f), pixel_format(rgba_format),
                                   ctypes.addressof(o), len(out))
    del keep, o
    _check(st)
    return bytes(out)


def rgba_to_nv12(rgba_bytes, w: int, h: int, fmt: YuvFormat | None = None, rgba_format="rgba", device: int = 0) -> bytes:
    """One host RGBA8 frame -> its tight NV12 frame (nus_rgba8_to_nv12)."""
    addr, n, keep = _as_buffer(rgba_bytes)
    cap = int(w) * int(h) + 2 * ((int(w) + 1) // 2) * ((int(h) + 1) // 2) if int(w) > 0 and int(h) > 0 else 4
    out = bytearray(cap)
    o = (ctypes.c_ubyte * len(out)).from_buffer(out)
    f = (fmt or YuvFormat())._c()
    st = C.lib().nus_rgba8_to_nv12(int(device), addr, n, int(w), int(h), ctypes.addressof(f), pixel_format(rgba_format),
                                   ctypes.addressof(o), len(out))
    del keep, o
    _check(st)
    return bytes(out)


def i420_to_nv12_device(d_i420: int, w: int, h: int, d_nv12: int, n_frames: int = 1, i420_frame_stride: int = 0, nv12_frame_stride: int = 0,
                        stream: int = 0, layout: Nv12Layout | None = None) -> None:
    """Enqueue the repack of `n_frames` tight I420 device frames into NV12 frames on `stream` (nus_yuv420_to_nv12_device): bytes only."""
    keep, la = _layout(layout)
    _check(C.lib().nus_yuv420_to_nv12_device(d_i420 or None, int(i420_frame_stride), int(w), int(h), d_nv12 or None, la,
                                             int(nv12_frame_stride), int(n_frames), stream or None))
    del keep


def nv12_to_i420_device(d_nv12: int, w: int, h: int, d_i420: int, n_frames: int = 1, nv12_frame_stride: int = 0, i420_frame_stride: int = 0,
                        stream: int = 0, layout: Nv12Layout | None = None) -> None:
    """Enqueue the repack of `n_frames` NV12 device frames into tight I420 frames on `stream` (nus_nv12_to_yuv420_device)."""
    keep, la = _layout(layout)
    _check(C.lib().nus_nv12_to_yuv420_device(d_nv12 or None, la, int(nv12_frame_stride), int(w), int(h), d_i420 or None,
                                             int(i420_frame_stride), int(n_frames), stream or None))
    del keep


_MODE = {"fma": C.LANCZOS_FMA, "exact": C.LANCZOS_EXACT}


def _algorithm(value) -> int:
    from .upscaler import _ALGORITHM

    return _enum("algorithm", _ALGORITHM, value)


class YuvResizer:
    """Up-scales I420 frames plane by plane (nus_yuv_resizer of include/nuscaler_hip.h, where the contract is written): Y, U and V
    are resampled as single-channel images with `algorithm` "lanczos3" | "bicubic" | "triangle", chroma at the position `siting`
    ("center" | "left") gives it; `mode` "fma" | "exact".  All four dimensions even, no axis scaled down; equal sizes copy.
    ValueError for bad arguments, RuntimeError for what the library does not support (odd sizes, down-scaling, other algorithms)
    and for device errors."""

    def __init__(self, iw: int, ih: int, ow: int, oh: int, algorithm="lanczos3", siting="center", mode="fma", device: int = 0):
        alg, sit, md = _algorithm(algorithm), _enum("siting", _SITING, siting), _enum("mode", _MODE, mode)
        self._lib = C.lib()
        self._h = self._lib.nus_yuv_resizer_create()
        if not self._h:
            raise MemoryError("nus_yuv_resizer_create failed")
        _check(self._lib.nus_yuv_resizer_set_device(self._h, int(device)))
        _check(self._lib.nus_yuv_resizer_initialize(self._h, int(iw), int(ih), int(ow), int(oh), alg, sit, md))
        self.iw, self.ih, self.ow, self.oh = int(iw), int(ih), int(ow), int(oh)
        self.in_frame_bytes = self.iw * self.ih * 3 // 2
        self.out_frame_bytes = self.ow * self.oh * 3 // 2

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.nus_yuv_resizer_destroy(h)

    def resize_device(self, d_in: int, d_out: int, n_frames: int = 1, in_frame_stride: int = 0, out_frame_stride: int = 0,
                      stream: int = 0) -> None:
        """Enqueue the up-scale of `n_frames` device frames on `stream` (nus_yuv420_resize_device); strides in bytes, 0 = tight.
        The handle's first device call uploads its tables."""
        _check(self._lib.nus_yuv420_resize_device(self._h, d_in or None, int(in_frame_stride), d_out or None, int(out_frame_stride),
                                                  int(n_frames), stream or None))

    def resize(self, frame_bytes) -> bytes:
        """One host I420 frame -> the up-scaled frame (nus_yuv420_resize)."""
        addr, n, keep = _as_buffer(frame_bytes)
        out = bytearray(self.out_frame_bytes)
        o = (ctypes.c_ubyte * len(out)).from_buffer(out)
        st = self._lib.nus_yuv420_resize(self._h, addr, n, ctypes.addressof(o), len(out))
        del keep, o
        _check(st)
        return bytes(out)

    def resize_nv12_device(self, d_in: int, d_out: int, n_frames: int = 1, in_frame_stride: int = 0, out_frame_stride: int = 0,
                           stream: int = 0) -> None:
        """The same on tight NV12 device frames (nus_nv12_resize_device): resize_device's output with U and V interleaved, bit for
        bit.  Pitched surfaces go through the conversions or the repack."""
        _check(self._lib.nus_nv12_resize_device(self._h, d_in or None, int(in_frame_stride), d_out or None, int(out_frame_stride),
                                                int(n_frames), stream or None))

    def resize_nv12(self, frame_bytes) -> bytes:
        """One tight host NV12 frame -> the up-scaled NV12 frame (nus_nv12_resize)."""
        addr, n, keep = _as_buffer(frame_bytes)
        out = bytearray(self.out_frame_bytes)
        o = (ctypes.c_ubyte * len(out)).from_buffer(out)
        st = self._lib.nus_nv12_resize(self._h, addr, n, ctypes.addressof(o), len(out))
        del keep, o
        _check(st)
        return bytes(out)

    def export_axis(self, plane: int, axis: int):
        """(left int32 [out_n], ntaps uint32 [out_n], weights float32 [out_n, RESIZE_MAX_TAPS]) of plane 0 luma / 1 chroma, axis
        0 x / 1 y (nus_yuv_resizer_export_axis)."""
        import numpy as np

        if plane not in (0, 1) or axis not in (0, 1):
            raise ValueError(f"plane and axis must be 0 or 1, got {plane!r}, {axis!r}")
        n = ((self.ow, self.oh)[axis]) // (2 if plane else 1)
        left, ntaps = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        w = np.zeros((n, C.RESIZE_MAX_TAPS), np.float32)
        _check(self._lib.nus_yuv_resizer_export_axis(self._h, int(plane), int(axis), left.ctypes.data, ntaps.ctypes.data, w.ctypes.data))
        return left, ntaps, w
