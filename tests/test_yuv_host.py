"""The YUV 4:2:0 entry points without a GPU (nus_yuv420_frame_bytes, nus_yuv_coefficients, nus_yuv420_to_rgba8[_device],
nus_rgba8_to_yuv420[_device]): the exports and the header's prototypes, the coefficient tables against the contract's derivation,
every argument check (before any HIP call: the device addresses below are never dereferenced; the text begins with the entry
point's name), the frame size, the unchanged ABI version, and the Python wrappers' errors."""
import ctypes
import os

import numpy as np
import pytest

import _yuv as Y
from conftest import ROOT

NEW = ("nus_yuv420_frame_bytes", "nus_yuv_coefficients", "nus_yuv420_to_rgba8_device", "nus_rgba8_to_yuv420_device", "nus_yuv420_to_rgba8",
       "nus_rgba8_to_yuv420")
CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


def test_exports_header_and_abi(nsc, lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in nsc._capi.SIGNATURES), name
    raw = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    assert "#define NUS_ABI_VERSION 1\n" in raw and raw.count("NUS_ABI_VERSION") == 1  # the line as it was
    assert lib.nus_abi_version() == 1
    hdr = " ".join(raw.split())
    assert "size_t nus_yuv420_frame_bytes(uint32_t w, uint32_t h);" in hdr
    assert "int nus_yuv_coefficients(int matrix, int range, int32_t *to_yuv, int32_t *to_rgb);" in hdr
    assert ("int nus_yuv420_to_rgba8_device(const void *d_yuv, size_t yuv_frame_stride, uint32_t w, uint32_t h, const nus_yuv_format *fmt, "
            "int rgba_format, void *d_rgba, size_t rgba_frame_stride, uint32_t n_frames, void *stream);") in hdr
    assert ("int nus_rgba8_to_yuv420_device(const void *d_rgba, size_t rgba_frame_stride, uint32_t w, uint32_t h, const nus_yuv_format *fmt, "
            "int rgba_format, void *d_yuv, size_t yuv_frame_stride, uint32_t n_frames, void *stream);") in hdr
    assert ("int nus_yuv420_to_rgba8(int device, const uint8_t *yuv, size_t yuv_len, uint32_t w, uint32_t h, const nus_yuv_format *fmt, "
            "int rgba_format, uint8_t *rgba, size_t rgba_cap);") in hdr
    assert ("int nus_rgba8_to_yuv420(int device, const uint8_t *rgba, size_t rgba_len, uint32_t w, uint32_t h, const nus_yuv_format *fmt, "
            "int rgba_format, uint8_t *yuv, size_t yuv_cap);") in hdr
    assert "BUILD-DEFINED" in hdr[hdr.index("YUV 4:2:0 frames"):hdr.index("typedef enum nus_yuv_matrix")]
    for text in ("NUS_YUV_MATRIX_BT601 = 0", "NUS_YUV_MATRIX_BT709 = 1", "NUS_YUV_RANGE_LIMITED = 0", "NUS_YUV_RANGE_FULL = 1",
                 "NUS_YUV_SITING_CENTER = 0", "NUS_YUV_SITING_LEFT = 1", "NUS_YUV_CHROMA_NEAREST = 0", "NUS_YUV_CHROMA_BILINEAR = 1"):
        assert text in hdr, text
    C = nsc._capi
    assert (C.YUV_MATRIX_BT601, C.YUV_MATRIX_BT709, C.YUV_RANGE_LIMITED, C.YUV_RANGE_FULL) == (0, 1, 0, 1)
    assert (C.YUV_SITING_CENTER, C.YUV_SITING_LEFT, C.YUV_CHROMA_NEAREST, C.YUV_CHROMA_BILINEAR) == (0, 1, 0, 1)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "nus_k_yuv.hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0] and "nus_yuv.cpp" in mk.split("HOST", 1)[1].split("\n", 1)[0]
    head = open(os.path.join(CSRC, "nus_k_yuv.hip")).read().split("#include", 1)[0]
    assert "BUILD-DEFINED" in head and "no LDS, no atomics, no scratch" in head


@pytest.mark.parametrize("matrix", (0, 1))
@pytest.mark.parametrize("rng", (0, 1))
def test_coefficients_are_the_derivation(nsc, lib, matrix, rng):
    a, b = (ctypes.c_int32 * 9)(), (ctypes.c_int32 * 5)()
    assert lib.nus_yuv_coefficients(matrix, rng, ctypes.addressof(a), ctypes.addressof(b)) == nsc._capi.OK
    want_yuv, want_rgb = Y.coefficients(matrix, rng)
    assert list(a) == want_yuv and list(b) == want_rgb
    # the derivation itself, spelled with the header's letters
    kr, kb = ((0.299, 0.114), (0.2126, 0.0722))[matrix]
    kg = 1 - kr - kb
    ys, cs = ((219, 224), (255, 255))[rng]
    q = lambda x: int(np.floor(x * 16384 + 0.5))
    near = lambda got, x: abs(got - x * 16384) <= 0.5 + 1e-6
    assert all(near(g, k * ys / 255) for g, k in zip(a[0:3], (kr, kg, kb)))
    assert all(near(g, k / (2 * (1 - kb)) * cs / 255) for g, k in zip(a[3:6], (-kr, -kg, 1 - kb)))
    assert all(near(g, k / (2 * (1 - kr)) * cs / 255) for g, k in zip(a[6:9], (1 - kr, -kg, -kb)))
    assert list(b) == [q(255 / ys), q(2 * (1 - kr) * 255 / cs), q(2 * (1 - kb) * 255 / cs), q(-2 * kb * (1 - kb) / kg * 255 / cs),
                       q(-2 * kr * (1 - kr) / kg * 255 / cs)]
    if rng == 1:
        assert sum(a[0:3]) == 16384  # full-range white is exactly 255
        assert a[5] == 8192 and a[6] == 8192 and b[0] == 16384
    assert a[3] + a[4] + a[5] in (-1, 0, 1) and a[6] + a[7] + a[8] in (-1, 0, 1)  # grey has no chroma, up to the rounding of Q
    assert nsc.yuv.coefficients(("bt601", "bt709")[matrix], ("limited", "full")[rng]) == (want_yuv, want_rgb)


def test_coefficients_check_their_arguments(nsc, lib):
    a, b = (ctypes.c_int32 * 9)(), (ctypes.c_int32 * 5)()
    inv = nsc._capi.ERR_INVALID_ARGUMENT
    for args, text in (((2, 0, ctypes.addressof(a), ctypes.addressof(b)), "unknown matrix 2"), ((0, -1, ctypes.addressof(a), ctypes.addressof(b)), "unknown range -1"),
                       ((0, 0, None, ctypes.addressof(b)), "null pointer"), ((0, 0, ctypes.addressof(a), None), "null pointer")):
        assert lib.nus_yuv_coefficients(*args) == inv
        assert nsc._capi.last_error() == "nus_yuv_coefficients: " + text


def test_frame_bytes(nsc, lib):
    for (w, h), want in (((1, 1), 3), ((2, 2), 6), ((3, 5), 27), ((1920, 1080), 3110400)):
        assert lib.nus_yuv420_frame_bytes(w, h) == want == Y.frame_bytes(w, h) == nsc.yuv.frame_bytes(w, h)
    for w, h, text in ((0, 4, "width and height must be non-zero"), (4, 0, "width and height must be non-zero"), (1 << 16, 1 << 15, "too large"),
                       (2, 524281, "height above 524280")):
        assert lib.nus_yuv420_frame_bytes(w, h) == 0
        msg = nsc._capi.last_error()
        assert msg.startswith("nus_yuv420_frame_bytes: ") and text in msg, msg
        with pytest.raises(ValueError, match="nus_yuv420_frame_bytes"):
            nsc.yuv.frame_bytes(w, h)
    assert lib.nus_yuv420_frame_bytes(2, 524280) == 2 * 524280 * 3 // 2


def _fmt(nsc, matrix=1, rng=0, siting=0, chroma=1):
    return nsc.yuv._Format(matrix, rng, siting, chroma)


@pytest.mark.parametrize("to_rgba", (True, False))
def test_device_entry_points_check_their_arguments_before_any_hip_call(nsc, lib, to_rgba):
    ok, inv = nsc._capi.OK, nsc._capi.ERR_INVALID_ARGUMENT
    name = "nus_yuv420_to_rgba8_device" if to_rgba else "nus_rgba8_to_yuv420_device"
    fn = getattr(lib, name)
    w, h = 6, 4
    yb, fb = 36, 96
    YUV, RGBA = 0x10000, 0x20000  # never dereferenced: every call below is refused first
    good = _fmt(nsc)

    def call(yuv=YUV, ys=0, w_=w, h_=h, f=good, pf=0, rgba=RGBA, rs=0, n=1):
        fa = ctypes.addressof(f) if f is not None else None
        return fn(yuv, ys, w_, h_, fa, pf, rgba, rs, n, None) if to_rgba else fn(rgba, rs, w_, h_, fa, pf, yuv, ys, n, None)

    def refused(text, **kw):
        assert call(**kw) == inv, kw
        msg = nsc._capi.last_error()
        assert msg.startswith(name + ": "), msg
        assert text in msg, msg

    refused("null pointer", yuv=None)
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
    refused(f"yuv_frame_stride must be 0 or at least {yb}", ys=yb - 1)
    refused("4-byte aligned", rgba=RGBA + 2)
    # the YUV side has no alignment rule, and an odd stride is a stride: these pass every check and stop at the device
    if nsc._capi.device_count() == 0:
        for kw in (dict(yuv=YUV + 1), dict(ys=yb + 1, n=2), dict(rs=fb + 4, n=2)):
            assert call(**kw) == nsc._capi.ERR_NO_DEVICE, kw
            assert nsc._capi.last_error() == name + ": no HIP device available"
    assert ok == 0


@pytest.mark.parametrize("to_rgba", (True, False))
def test_host_entry_points_check_their_arguments_before_any_hip_call(nsc, lib, to_rgba):
    inv, size = nsc._capi.ERR_INVALID_ARGUMENT, nsc._capi.ERR_SIZE_MISMATCH
    name = "nus_yuv420_to_rgba8" if to_rgba else "nus_rgba8_to_yuv420"
    fn = getattr(lib, name)
    w, h = 6, 4
    yb, fb = 36, 96
    src_n, dst_n = (yb, fb) if to_rgba else (fb, yb)
    src, dst = (ctypes.c_ubyte * src_n)(), (ctypes.c_ubyte * dst_n)()
    good = _fmt(nsc)

    def call(s=ctypes.addressof(src), sl=src_n, w_=w, h_=h, f=good, pf=0, d=ctypes.addressof(dst), cap=dst_n, device=0):
        return fn(device, s, sl, w_, h_, ctypes.addressof(f) if f is not None else None, pf, d, cap)

    def refused(status, text, **kw):
        assert call(**kw) == status, kw
        msg = nsc._capi.last_error()
        assert msg.startswith(name + ": ") and text in msg, msg

    refused(inv, "null pointer", s=None)
    refused(inv, "null pointer", d=None)
    refused(inv, "null pointer", f=None)
    refused(inv, "width and height must be non-zero", w_=0)
    refused(inv, "unknown matrix 3", f=_fmt(nsc, matrix=3))
    refused(inv, "unknown siting -2", f=_fmt(nsc, siting=-2))
    refused(inv, "unknown pixel format 9", pf=9)
    src_name, dst_name = ("yuv_len", "rgba_cap") if to_rgba else ("rgba_len", "yuv_cap")
    refused(size, f"{src_name} ({src_n - 1}) does not match the frame size ({src_n} for 6x4)", sl=src_n - 1)
    refused(size, f"{src_name} ({src_n + 1}) does not match the frame size ({src_n} for 6x4)", sl=src_n + 1)
    refused(size, f"{dst_name} ({dst_n - 1}) is below the frame size ({dst_n} for 6x4)", cap=dst_n - 1)
    if nsc._capi.device_count() == 0:
        assert call() == nsc._capi.ERR_NO_DEVICE and nsc._capi.last_error() == name + ": no HIP device available"
    # the Python wrappers raise ValueError with the library's text
    wrap = nsc.yuv.to_rgba if to_rgba else nsc.yuv.to_yuv
    with pytest.raises(ValueError, match=name + ": " + src_name):
        wrap(bytes(src_n - 1), w, h)
    with pytest.raises(ValueError, match="unknown pixel format"):
        wrap(bytes(src_n), w, h, rgba_format=5)


def test_python_format_and_device_wrappers(nsc):
    f = nsc.yuv.YuvFormat()
    assert (f.matrix, f.range, f.siting, f.chroma) == (1, 0, 0, 1)
    assert repr(nsc.yuv.YuvFormat("bt601", "full", "left", "nearest")) == "YuvFormat(matrix='bt601', range='full', siting='left', chroma='nearest')"
    for kw in (dict(matrix="bt2020"), dict(range="pc"), dict(siting="top"), dict(chroma="cubic"), dict(matrix=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            nsc.yuv.YuvFormat(**kw)
    with pytest.raises(ValueError, match="nus_yuv420_to_rgba8_device: null pointer"):
        nsc.yuv.to_rgba_device(0, 6, 4, 0x20000)
    with pytest.raises(ValueError, match="nus_rgba8_to_yuv420_device: n_frames must be at least 1"):
        nsc.yuv.to_yuv_device(0x20000, 6, 4, 0x10000, n_frames=0)
    with pytest.raises(ValueError, match="nus_rgba8_to_yuv420_device: unknown matrix 5"):
        nsc.yuv.to_yuv_device(0x20000, 6, 4, 0x10000, nsc.yuv.YuvFormat(matrix=5))
    with pytest.raises(ValueError, match="yuv_frame_stride must be 0 or at least 36"):
        nsc.yuv.to_rgba_device(0x10000, 6, 4, 0x20000, yuv_frame_stride=35)
