"""The NV12 entry points without a GPU (nus_nv12_frame_bytes, nus_nv12_to_rgba8[_device], nus_rgba8_to_nv12[_device],
nus_yuv420_to_nv12_device, nus_nv12_to_yuv420_device, nus_nv12_resize[_device] and their wrappers in nu_scaler_amd.yuv): the exports,
the header's prototypes and the unchanged ABI version, the Makefile lists; the frame size and the layout rule; every argument check
(before any HIP call: the device addresses below are never dereferenced; the text begins with the entry point's name); the Python
wrappers' errors; the numpy layout yardstick on itself; and the scan that decides how wide a union the pair row kernel is compiled
for (nus_k_nv12_resize.hip)."""
import ctypes
import os

import numpy as np
import pytest

import _nv12 as N
import _plane_resample64 as P
import _yuv as Y
from conftest import ROOT

NEW = ("nus_nv12_frame_bytes", "nus_nv12_to_rgba8_device", "nus_rgba8_to_nv12_device", "nus_nv12_to_rgba8", "nus_rgba8_to_nv12",
       "nus_yuv420_to_nv12_device", "nus_nv12_to_yuv420_device", "nus_nv12_resize_device", "nus_nv12_resize")
CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")
FILTERS = ((0, "lanczos3"), (1, "bicubic"), (2, "triangle"))


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


@pytest.fixture()
def handle(lib):
    h = lib.nus_yuv_resizer_create()
    assert h
    yield h
    lib.nus_yuv_resizer_destroy(h)


def _fmt(nsc, matrix=1, rng=0, siting=0, chroma=1):
    return nsc.yuv._Format(matrix, rng, siting, chroma)


def _lay(nsc, pitch=0, uv_offset=0):
    return nsc.yuv._Layout(pitch, uv_offset)


def test_exports_header_abi_and_makefile(nsc, lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in nsc._capi.SIGNATURES), name
    raw = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    assert "#define NUS_ABI_VERSION 1\n" in raw and raw.count("NUS_ABI_VERSION") == 1
    assert lib.nus_abi_version() == 1
    hdr = " ".join(raw.split())
    for proto in (
            "typedef struct nus_nv12_layout { size_t pitch; /* bytes between rows, of the Y plane and of the UV plane alike; 0 = tight */ "
            "size_t uv_offset; /* bytes from the frame's base to its UV plane; 0 = directly behind the Y rows */ } nus_nv12_layout;",
            "size_t nus_nv12_frame_bytes(uint32_t w, uint32_t h, const nus_nv12_layout *layout);",
            "int nus_nv12_to_rgba8_device(const void *d_nv12, const nus_nv12_layout *layout, size_t nv12_frame_stride, uint32_t w, uint32_t h, "
            "const nus_yuv_format *fmt, int rgba_format, void *d_rgba, size_t rgba_frame_stride, uint32_t n_frames, void *stream);",
            "int nus_rgba8_to_nv12_device(const void *d_rgba, size_t rgba_frame_stride, uint32_t w, uint32_t h, const nus_yuv_format *fmt, "
            "int rgba_format, void *d_nv12, const nus_nv12_layout *layout, size_t nv12_frame_stride, uint32_t n_frames, void *stream);",
            "int nus_nv12_to_rgba8(int device, const uint8_t *nv12, size_t nv12_len, uint32_t w, uint32_t h, const nus_yuv_format *fmt, "
            "int rgba_format, uint8_t *rgba, size_t rgba_cap);",
            "int nus_rgba8_to_nv12(int device, const uint8_t *rgba, size_t rgba_len, uint32_t w, uint32_t h, const nus_yuv_format *fmt, "
            "int rgba_format, uint8_t *nv12, size_t nv12_cap);",
            "int nus_yuv420_to_nv12_device(const void *d_i420, size_t i420_frame_stride, uint32_t w, uint32_t h, void *d_nv12, "
            "const nus_nv12_layout *layout, size_t nv12_frame_stride, uint32_t n_frames, void *stream);",
            "int nus_nv12_to_yuv420_device(const void *d_nv12, const nus_nv12_layout *layout, size_t nv12_frame_stride, uint32_t w, uint32_t h, "
            "void *d_i420, size_t i420_frame_stride, uint32_t n_frames, void *stream);",
            "int nus_nv12_resize_device(nus_yuv_resizer *h, const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride, "
            "uint32_t n_frames, void *stream);",
            "int nus_nv12_resize(nus_yuv_resizer *h, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);"):
        assert proto in hdr, proto
    # the section stands behind the planar up-scaler's, is marked as this build's own and says what is still out
    at = hdr.index("NV12 frames: conversions")
    assert at > hdr.index("int nus_yuv420_resize(nus_yuv_resizer *h")
    sec = hdr[at:hdr.index("typedef struct nus_nv12_layout")]
    for text in ("BUILD-DEFINED", "NV21", "P010", "4:2:2", "pitched resize", "Y4M has no tag", "command-line tool", "Row padding, the gap between the planes"):
        assert text in sec, text
    assert "No NV12" not in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    kernels, hdrs = mk.split("KERNELS", 1)[1].split("\n", 1)[0], mk.split("HDRS", 1)[1].split("\n", 1)[0]
    assert "nus_k_nv12.hip" in kernels and "nus_k_nv12_resize.hip" in kernels and "nus_yuv_device.hpp" in hdrs
    # the arithmetic is shared, not copied: both conversion units include the device header and neither spells the functions out
    shared = open(os.path.join(CSRC, "nus_yuv_device.hpp")).read()
    for fn in ("yuv_pixel(", "chroma_h(", "luma_of(", "chroma_of(", "lane_copies("):
        assert shared.count("uint32_t " + fn) + shared.count("int " + fn) + shared.count("void " + fn) == 1, fn
    assert 'asm volatile("" : "+v"(r), "+v"(g), "+v"(b));' in shared
    for unit in ("nus_k_yuv.hip", "nus_k_nv12.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert '#include "nus_yuv_device.hpp"' in text, unit
        for fn in ("yuv_pixel(int", "chroma_h(bool", "luma_of(uint32_t", "chroma_of(uint32_t", "lane_copies(YuvTables"):
            assert fn not in text, (unit, fn)
    for unit, words in (("nus_k_nv12.hip", ("BUILD-DEFINED", "no LDS, no atomics, no scratch")), ("nus_k_nv12_resize.hip", ("BUILD-DEFINED", "no scratch"))):
        head = open(os.path.join(CSRC, unit)).read().split("#include", 1)[0]
        assert all(x in head for x in words), unit


def test_frame_bytes_and_the_layout_rule(nsc, lib):
    C = nsc._capi
    for w, h in ((1, 1), (2, 2), (3, 5), (5, 2), (6, 4), (1920, 1080)):
        want = Y.frame_bytes(w, h)
        assert lib.nus_nv12_frame_bytes(w, h, None) == want == lib.nus_yuv420_frame_bytes(w, h) == nsc.yuv.nv12_frame_bytes(w, h)
        z = _lay(nsc)
        assert lib.nus_nv12_frame_bytes(w, h, ctypes.addressof(z)) == want == nsc.yuv.nv12_frame_bytes(w, h, nsc.yuv.Nv12Layout())
        assert N.interleave(np.zeros(want, np.uint8), w, h).size == want
    for w, h, pitch, off, want in ((5, 3, 6, 0, 6 * 3 + 6 * 2), (5, 3, 6, 18, 30), (5, 3, 8, 31, 31 + 16), (32, 6, 64, 64 * 8, 512 + 192), (34, 5, 40, 203, 203 + 120),
                                   (1920, 1080, 2048, 2048 * 1088, 2048 * 1088 + 2048 * 540)):
        l = _lay(nsc, pitch, off)
        assert lib.nus_nv12_frame_bytes(w, h, ctypes.addressof(l)) == want == nsc.yuv.nv12_frame_bytes(w, h, nsc.yuv.Nv12Layout(pitch, off))
        assert N.interleave(np.zeros(Y.frame_bytes(w, h), np.uint8), w, h, pitch, off).size == want
    for w, h, pitch, off, text in ((5, 3, 5, 0, "pitch must be 0 or at least 6"), (6, 4, 4, 0, "pitch must be 0 or at least 6"), (6, 4, 8, 31, "uv_offset must be 0 or at least 32"),
                                   (6, 4, 8, 1, "uv_offset must be 0 or at least 32"), (6, 4, 0, 24, "pitch 0 (tight) must have uv_offset 0"),
                                   (6, 4, 1 << 41, 0, "too large"), (0, 4, 0, 0, "width and height must be non-zero"), (2, 524281, 0, 0, "height above 524280")):
        l = _lay(nsc, pitch, off)
        assert lib.nus_nv12_frame_bytes(w, h, ctypes.addressof(l)) == 0
        msg = C.last_error()
        assert msg.startswith("nus_nv12_frame_bytes: ") and text in msg, msg
        with pytest.raises(ValueError, match="nus_nv12_frame_bytes"):
            nsc.yuv.nv12_frame_bytes(w, h, nsc.yuv.Nv12Layout(pitch, off))


def test_the_layout_yardstick_on_itself():
    rng = np.random.default_rng(12)
    for w, h, pitch, off in ((5, 3, 0, 0), (6, 4, 0, 0), (5, 3, 9, 0), (6, 4, 8, 37), (1, 1, 0, 0), (1, 1, 2, 5)):
        x = rng.integers(0, 256, Y.frame_bytes(w, h), dtype=np.uint8)
        nv = N.interleave(x, w, h, pitch, off, fill=0x5C)
        np.testing.assert_array_equal(N.deinterleave(nv, w, h, pitch, off), x)
        yp, up, vp = Y.split(x, w, h)
        o = off or (pitch or w) * h
        p = pitch or 2 * ((w + 1) // 2)
        assert nv[0] == yp[0, 0] and nv[o] == up[0, 0] and nv[o + 1] == vp[0, 0]
        assert nv[o + p * (up.shape[0] - 1) + 2 * (up.shape[1] - 1) + 1] == vp[-1, -1]
    x = np.arange(6, dtype=np.uint8)  # 2 x 2: Y 0 1 2 3, U 4, V 5
    np.testing.assert_array_equal(N.interleave(x, 2, 2), [0, 1, 2, 3, 4, 5])
    np.testing.assert_array_equal(N.interleave(np.arange(12, dtype=np.uint8), 4, 2), [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 9, 11])
    np.testing.assert_array_equal(N.interleave(np.arange(12, dtype=np.uint8), 4, 2, 6, 14, 99), [0, 1, 2, 3, 99, 99, 4, 5, 6, 7, 99, 99, 99, 99, 8, 10, 9, 11, 99, 99])


@pytest.mark.parametrize("to_rgba", (True, False))
def test_conversion_device_entry_points_check_their_arguments_before_any_hip_call(nsc, lib, to_rgba):
    C = nsc._capi
    inv = C.ERR_INVALID_ARGUMENT
    name = "nus_nv12_to_rgba8_device" if to_rgba else "nus_rgba8_to_nv12_device"
    fn = getattr(lib, name)
    w, h = 6, 4
    nb, fb = 36, 96
    NV, RGBA = 0x10000, 0x20000  # never dereferenced: every call below is refused first
    good = _fmt(nsc)

    def call(nv=NV, lay=None, ns=0, w_=w, h_=h, f=good, pf=0, rgba=RGBA, rs=0, n=1):
        fa = ctypes.addressof(f) if f is not None else None
        la = ctypes.addressof(lay) if lay is not None else None
        return fn(nv, la, ns, w_, h_, fa, pf, rgba, rs, n, None) if to_rgba else fn(rgba, rs, w_, h_, fa, pf, nv, la, ns, n, None)

    def refused(text, **kw):
        assert call(**kw) == inv, kw
        msg = C.last_error()
        assert msg.startswith(name + ": "), msg
        assert text in msg, msg

    refused("null pointer", nv=None)
    refused("null pointer", rgba=None)
    refused("null pointer", f=None)
    refused("width and height must be non-zero", w_=0)
    refused("width and height must be non-zero", h_=0)
    refused("too large", w_=1 << 16, h_=1 << 15)
    refused("height above 524280", w_=2, h_=524282)
    refused("unknown matrix 2", f=_fmt(nsc, matrix=2))
    refused("unknown range -1", f=_fmt(nsc, rng=-1))
    refused("unknown siting 2", f=_fmt(nsc, siting=2))
    refused("unknown chroma_filter 7", f=_fmt(nsc, chroma=7))
    refused("unknown pixel format 4", pf=4)
    refused("unknown pixel format -1", pf=-1)
    refused("n_frames must be at least 1", n=0)
    refused(f"rgba_frame_stride must be 0 or a multiple of 4 of at least {fb}", rs=fb - 4)
    refused(f"rgba_frame_stride must be 0 or a multiple of 4 of at least {fb}", rs=fb + 2)
    refused(f"nv12_frame_stride must be 0 or at least {nb}", ns=nb - 1)
    refused("4-byte aligned", rgba=RGBA + 2)
    refused("pitch must be 0 or at least 6, got 5", lay=_lay(nsc, 5))
    refused("uv_offset must be 0 or at least 32, got 31", lay=_lay(nsc, 8, 31))
    refused("pitch 0 (tight) must have uv_offset 0", lay=_lay(nsc, 0, 24))
    refused("nv12_frame_stride must be 0 or at least 48, got 47", lay=_lay(nsc, 8), ns=47)  # the pitched frame: 8 * 4 + 8 * 2
    refused("nv12_frame_stride must be 0 or at least 56, got 55", lay=_lay(nsc, 8, 40), ns=55)
    # the NV12 side has no alignment rule, and an odd pitch is a pitch: these pass every check and stop at the device
    if C.device_count() == 0:
        for kw in (dict(nv=NV + 1), dict(ns=nb + 1, n=2), dict(rs=fb + 4, n=2), dict(lay=_lay(nsc, 7)), dict(lay=_lay(nsc, 8, 33), ns=49, n=2)):
            assert call(**kw) == C.ERR_NO_DEVICE, kw
            assert C.last_error() == name + ": no HIP device available"


@pytest.mark.parametrize("to_nv12", (True, False))
def test_repack_entry_points_check_their_arguments_before_any_hip_call(nsc, lib, to_nv12):
    C = nsc._capi
    inv = C.ERR_INVALID_ARGUMENT
    name = "nus_yuv420_to_nv12_device" if to_nv12 else "nus_nv12_to_yuv420_device"
    fn = getattr(lib, name)
    w, h, nb = 6, 4, 36
    I420, NV = 0x10000, 0x20000

    def call(i420=I420, is_=0, w_=w, h_=h, nv=NV, lay=None, ns=0, n=1):
        la = ctypes.addressof(lay) if lay is not None else None
        return fn(i420, is_, w_, h_, nv, la, ns, n, None) if to_nv12 else fn(nv, la, ns, w_, h_, i420, is_, n, None)

    def refused(text, **kw):
        assert call(**kw) == inv, kw
        msg = C.last_error()
        assert msg.startswith(name + ": ") and text in msg, msg

    refused("null pointer", i420=None)
    refused("null pointer", nv=None)
    refused("width and height must be non-zero", w_=0)
    refused("width and height must be non-zero", h_=0)
    refused("too large", w_=1 << 16, h_=1 << 15)
    refused("height above 524280", w_=2, h_=524282)
    refused("n_frames must be at least 1", n=0)
    refused(f"i420_frame_stride must be 0 or at least {nb}, got {nb - 1}", is_=nb - 1)
    refused(f"nv12_frame_stride must be 0 or at least {nb}, got {nb - 1}", ns=nb - 1)
    refused("pitch must be 0 or at least 6, got 4", lay=_lay(nsc, 4))
    refused("uv_offset must be 0 or at least 28, got 27", lay=_lay(nsc, 7, 27))
    refused("pitch 0 (tight) must have uv_offset 0", lay=_lay(nsc, 0, 1))
    refused("nv12_frame_stride must be 0 or at least 42, got 41", lay=_lay(nsc, 7), ns=41)
    if C.device_count() == 0:
        for kw in (dict(i420=I420 + 1), dict(nv=NV + 3), dict(is_=nb + 1, n=2), dict(lay=_lay(nsc, 7, 29), ns=44, n=2)):
            assert call(**kw) == C.ERR_NO_DEVICE, kw
            assert C.last_error() == name + ": no HIP device available"


@pytest.mark.parametrize("to_rgba", (True, False))
def test_conversion_host_entry_points_check_their_arguments_before_any_hip_call(nsc, lib, to_rgba):
    C = nsc._capi
    inv, size = C.ERR_INVALID_ARGUMENT, C.ERR_SIZE_MISMATCH
    name = "nus_nv12_to_rgba8" if to_rgba else "nus_rgba8_to_nv12"
    fn = getattr(lib, name)
    w, h = 6, 4
    nb, fb = 36, 96
    src_n, dst_n = (nb, fb) if to_rgba else (fb, nb)
    src, dst = (ctypes.c_ubyte * src_n)(), (ctypes.c_ubyte * dst_n)()
    good = _fmt(nsc)

    def call(s=ctypes.addressof(src), sl=src_n, w_=w, h_=h, f=good, pf=0, d=ctypes.addressof(dst), cap=dst_n, device=0):
        return fn(device, s, sl, w_, h_, ctypes.addressof(f) if f is not None else None, pf, d, cap)

    def refused(status, text, **kw):
        assert call(**kw) == status, kw
        msg = C.last_error()
        assert msg.startswith(name + ": ") and text in msg, msg

    refused(inv, "null pointer", s=None)
    refused(inv, "null pointer", d=None)
    refused(inv, "null pointer", f=None)
    refused(inv, "width and height must be non-zero", w_=0)
    refused(inv, "too large", w_=1 << 16, h_=1 << 15)
    refused(inv, "unknown matrix 3", f=_fmt(nsc, matrix=3))
    refused(inv, "unknown siting -2", f=_fmt(nsc, siting=-2))
    refused(inv, "unknown pixel format 9", pf=9)
    src_name, dst_name = ("nv12_len", "rgba_cap") if to_rgba else ("rgba_len", "nv12_cap")
    refused(size, f"{src_name} ({src_n - 1}) does not match the frame size ({src_n} for 6x4)", sl=src_n - 1)
    refused(size, f"{src_name} ({src_n + 1}) does not match the frame size ({src_n} for 6x4)", sl=src_n + 1)
    refused(size, f"{dst_name} ({dst_n - 1}) is below the frame size ({dst_n} for 6x4)", cap=dst_n - 1)
    if C.device_count() == 0:
        assert call() == C.ERR_NO_DEVICE and C.last_error() == name + ": no HIP device available"
    wrap = nsc.yuv.nv12_to_rgba if to_rgba else nsc.yuv.rgba_to_nv12
    with pytest.raises(ValueError, match=name + ": " + src_name):
        wrap(bytes(src_n - 1), w, h)
    with pytest.raises(ValueError, match="unknown pixel format"):
        wrap(bytes(src_n), w, h, rgba_format=5)


def test_resize_entry_points_check_their_arguments_before_any_hip_call(nsc, lib, handle):
    C = nsc._capi
    IN, OUT = 0x10000, 0x20000
    in_b, out_b = 16 * 8 * 3 // 2, 32 * 16 * 3 // 2
    src, dst = (ctypes.c_ubyte * (in_b + 1))(), (ctypes.c_ubyte * out_b)()

    def dev(status, text, h=handle, d_in=IN, si=0, d_out=OUT, so=0, n=1):
        assert lib.nus_nv12_resize_device(h, d_in, si, d_out, so, n, None) == status, text
        msg = C.last_error()
        assert msg.startswith("nus_nv12_resize_device: ") and text in msg, msg

    def host(status, text, h=handle, s=ctypes.addressof(src), sl=in_b, d=ctypes.addressof(dst), cap=out_b):
        assert lib.nus_nv12_resize(h, s, sl, d, cap) == status, text
        msg = C.last_error()
        assert msg.startswith("nus_nv12_resize: ") and text in msg, msg

    dev(C.ERR_INVALID_ARGUMENT, "null handle", h=None)
    host(C.ERR_INVALID_ARGUMENT, "null handle", h=None)
    dev(C.ERR_NOT_INITIALIZED, "not initialized")
    host(C.ERR_NOT_INITIALIZED, "not initialized")
    assert lib.nus_yuv_resizer_initialize(handle, 16, 8, 32, 16, C.ALG_LANCZOS3, 1, 0) == C.OK
    dev(C.ERR_INVALID_ARGUMENT, "null pointer", d_in=None)
    dev(C.ERR_INVALID_ARGUMENT, "null pointer", d_out=None)
    dev(C.ERR_INVALID_ARGUMENT, "n_frames must be at least 1", n=0)
    dev(C.ERR_INVALID_ARGUMENT, f"in_frame_stride must be 0 or at least {in_b}, got {in_b - 1}", si=in_b - 1)
    dev(C.ERR_INVALID_ARGUMENT, f"out_frame_stride must be 0 or at least {out_b}, got {out_b - 1}", so=out_b - 1)
    host(C.ERR_INVALID_ARGUMENT, "null pointer", s=None)
    host(C.ERR_INVALID_ARGUMENT, "null pointer", d=None)
    host(C.ERR_SIZE_MISMATCH, f"in_len ({in_b - 1}) does not match the frame size ({in_b} for 16x8)", sl=in_b - 1)
    host(C.ERR_SIZE_MISMATCH, f"in_len ({in_b + 1}) does not match the frame size ({in_b} for 16x8)", sl=in_b + 1)
    host(C.ERR_SIZE_MISMATCH, f"out_cap ({out_b - 1}) is below the frame size ({out_b} for 32x16)", cap=out_b - 1)
    if C.device_count() == 0:
        for kw in (dict(), dict(d_in=IN + 1), dict(si=in_b + 1, n=2), dict(so=out_b + 3, n=2)):
            dev(C.ERR_NO_DEVICE, "no HIP device available", **kw)
        host(C.ERR_NO_DEVICE, "no HIP device available")
    r = nsc.yuv.YuvResizer(16, 8, 32, 16)
    with pytest.raises(ValueError, match="nus_nv12_resize_device: null pointer"):
        r.resize_nv12_device(0, OUT)
    with pytest.raises(ValueError, match="nus_nv12_resize_device: n_frames must be at least 1"):
        r.resize_nv12_device(IN, OUT, n_frames=0)
    with pytest.raises(ValueError, match=f"out_frame_stride must be 0 or at least {out_b}"):
        r.resize_nv12_device(IN, OUT, out_frame_stride=8)
    with pytest.raises(ValueError, match="nus_nv12_resize: in_len"):
        r.resize_nv12(bytes(in_b - 1))


def test_python_wrappers_map_their_errors(nsc):
    L = nsc.yuv.Nv12Layout
    assert (L().pitch, L().uv_offset) == (0, 0) and repr(L(64, 512)) == "Nv12Layout(pitch=64, uv_offset=512)"
    for kw in (dict(pitch=-1), dict(uv_offset=-8), dict(pitch=1.5), dict(pitch=True), dict(uv_offset="0")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            L(**kw)
    with pytest.raises(ValueError, match="layout must be an Nv12Layout or None"):
        nsc.yuv.nv12_to_rgba_device(0x10000, 6, 4, 0x20000, layout=(8, 0))
    with pytest.raises(ValueError, match="nus_nv12_to_rgba8_device: null pointer"):
        nsc.yuv.nv12_to_rgba_device(0, 6, 4, 0x20000)
    with pytest.raises(ValueError, match="nus_rgba8_to_nv12_device: n_frames must be at least 1"):
        nsc.yuv.rgba_to_nv12_device(0x20000, 6, 4, 0x10000, n_frames=0)
    with pytest.raises(ValueError, match="nus_rgba8_to_nv12_device: unknown matrix 5"):
        nsc.yuv.rgba_to_nv12_device(0x20000, 6, 4, 0x10000, nsc.yuv.YuvFormat(matrix=5))
    with pytest.raises(ValueError, match="nv12_frame_stride must be 0 or at least 36"):
        nsc.yuv.nv12_to_rgba_device(0x10000, 6, 4, 0x20000, nv12_frame_stride=35)
    with pytest.raises(ValueError, match="nus_nv12_to_rgba8_device: pitch must be 0 or at least 6, got 5"):
        nsc.yuv.nv12_to_rgba_device(0x10000, 6, 4, 0x20000, layout=L(5))
    with pytest.raises(ValueError, match="nus_rgba8_to_nv12_device: uv_offset must be 0 or at least 32, got 8"):
        nsc.yuv.rgba_to_nv12_device(0x20000, 6, 4, 0x10000, layout=L(8, 8))
    with pytest.raises(ValueError, match="nus_yuv420_to_nv12_device: null pointer"):
        nsc.yuv.i420_to_nv12_device(0, 6, 4, 0x20000)
    with pytest.raises(ValueError, match="nus_yuv420_to_nv12_device: a layout with pitch 0 .tight. must have uv_offset 0, got 64"):
        nsc.yuv.i420_to_nv12_device(0x10000, 6, 4, 0x20000, layout=L(0, 64))
    with pytest.raises(ValueError, match="nus_nv12_to_yuv420_device: i420_frame_stride must be 0 or at least 36"):
        nsc.yuv.nv12_to_i420_device(0x20000, 6, 4, 0x10000, i420_frame_stride=12)
    with pytest.raises(ValueError, match="nus_nv12_to_yuv420_device: n_frames must be at least 1"):
        nsc.yuv.nv12_to_i420_device(0x20000, 6, 4, 0x10000, n_frames=0)
    if nsc._capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="nus_yuv420_to_nv12_device: no HIP device available"):
            nsc.yuv.i420_to_nv12_device(0x10000, 6, 4, 0x20000, layout=L(8, 40))


def _pair_geometry(left, ntaps, out_n):
    """(footprint bytes, union cells) of a chroma x axis in the pair row kernel, by the two loops of YuvResizer::initialize: the
    widest dword-aligned input footprint of a segment of 128 output cells, in bytes, and the widest union of the windows of a
    lane's run of two cells."""
    left, end = np.asarray(left, np.int64)[:out_n], np.asarray(left, np.int64)[:out_n] + np.asarray(ntaps, np.int64)[:out_n]
    ncols = 0
    for x0 in range(0, out_n, 128):
        xl = min(x0 + 128, out_n) - 1
        ncols = max(ncols, (2 * int(end[xl]) - ((2 * int(left[x0])) & ~3) + 3) & ~3)
    return ncols, int((end.reshape(-1, 2).max(axis=1) - left[::2]).max())


SCAN_IN = range(4, 1101, 4)  # every luma input width the row form takes; the chroma axis is half of it
SCAN_API_IN = tuple(range(4, 1101, 48)) + (1100,)


def _scan_api_out(in_n):  # the ten ratios closest to 1 and every eleventh output width above them
    return sorted(set(range(in_n, min(in_n + 40, 4 * in_n + 1), 4)) | set(range(in_n, 4 * in_n + 1, 44)))


@pytest.mark.parametrize("filt,alg", FILTERS)
def test_a_run_of_two_pairs_needs_at_most_taps_plus_one_columns(nsc, filt, alg):
    """How many UNION instances of k_pair_rows to compile, decided as the bound of k_plane_rows was: every chroma x axis that the
    pair row form takes -- luma widths multiples of 4, so chroma in_n = iw / 2 -> out_n = ow / 2 -- for luma input widths 4 .. 1100
    and output widths in .. 4 in, at both sample positions, from the float32 window restatement (_plane_resample64.windows):
    114 125 axes per filter and position.  1 133 of them are also built by the library and must give the restatement's windows
    exactly.  Found: Lanczos-3 7 taps and union 8, Catmull-Rom 5 and 6, Triangle 3 and 4 -- taps + 1, at either position.  So
    launch_pair_resize's one instance, UNION = 8 = kPairMaxUnion, covers the range and nothing wider is compiled."""
    expected = {0: (7, 8), 1: (5, 6), 2: (3, 4)}[filt]
    axes = checked = 0
    for phi, siting in ((0.5, "center"), (0.25, "left")):
        taps = union = 0
        for iw in SCAN_IN:
            in_n = iw // 2
            outs = np.arange(iw, 4 * iw + 1, 4) // 2
            for c in range(0, len(outs), 48):
                lo, n, valid = P.windows(in_n, outs[c:c + 48], filt, phi)
                end = lo + n
                un = (end.reshape(len(end), -1, 2).max(axis=2) - lo[:, ::2])[valid[:, ::2]]
                assert (n[valid] >= 1).all() and (un >= 1).all()
                taps, union = max(taps, int(n.max())), max(union, int(un.max()))
            axes += len(outs)
            if iw in SCAN_API_IN:
                for ow in _scan_api_out(iw):
                    left, ntaps, _w = nsc.yuv.YuvResizer(iw, 2, ow, 2, alg, siting).export_axis(1, 0)
                    lo, n, _v = P.windows(in_n, [ow // 2], filt, phi)
                    np.testing.assert_array_equal(left, lo[0], err_msg=f"{alg} {iw}->{ow} {siting}")
                    np.testing.assert_array_equal(ntaps, n[0], err_msg=f"{alg} {iw}->{ow} {siting}")
                    u = _pair_geometry(left, ntaps, ow // 2)[1]
                    assert u == int(((lo[0] + n[0]).reshape(-1, 2).max(axis=1) - lo[0, ::2]).max())
                    assert u <= expected[1]
                    checked += 1
        print(f"{alg} phi {phi}: most taps {taps}, widest union of two {union}")
        assert union <= taps + 1 and taps <= 7 and union <= 8, (alg, phi, taps, union)
        assert (taps, union) == expected, (alg, phi, taps, union)
    assert axes == 2 * 114125 and checked == 2 * 1133, (axes, checked)
    kern = open(os.path.join(CSRC, "nus_kernels.hpp")).read()
    assert "constexpr uint32_t kPairMaxUnion = 8;" in kern
    unit = open(os.path.join(CSRC, "nus_k_nv12_resize.hip")).read()
    assert unit.count("k_pair_rows<true, 8>") == 1 and unit.count("k_pair_rows<false, 8>") == 1


def test_the_resize_cases_of_the_gpu_tests_are_what_they_say(nsc):
    """tests/test_gpu_nv12_resize.py names the chroma form of each shape; the numbers behind the names need no device."""
    import test_gpu_nv12_resize as T

    for shape, rows in T.SHAPES:
        iw, ih, ow, oh = shape
        assert ((iw % 4 == 0) and (ow % 4 == 0)) == rows, shape
        for siting in ("center", "left"):
            left, ntaps, _ = nsc.yuv.YuvResizer(iw, ih, ow, oh, "lanczos3", siting).export_axis(1, 0)
            if ow % 4 == 0:
                ncols, union = _pair_geometry(left, ntaps, ow // 2)
                assert 1 <= union <= 8 and ncols <= 4096, (shape, ncols, union)
    left, ntaps, _ = nsc.yuv.YuvResizer(504, 4, 512, 8, "lanczos3", "center").export_axis(1, 0)
    assert _pair_geometry(left, ntaps, 256)[0] >= 256  # a 256-byte footprint and more: the V pass sweeps twice
