"""The planar up-scaler of I420 frames without a GPU (nus_yuv_resizer_*, nus_yuv420_resize[_device], yuv.YuvResizer and the
`scale_domain` keyword of video.convert_y4m): the exports, the header's prototypes and the unchanged ABI version; every argument
check (before any HIP call: the device addresses below are never dereferenced; the text begins with the entry point's name); the
four axis tables against the oracle and the float32 restatement of tests/_plane_resample64.py; the restatement against the
oracle; the conversion's refusals and the CLI flag."""
import ctypes
import os

import numpy as np
import pytest

import _plane_resample64 as P
from conftest import ROOT

NEW = ("nus_yuv_resizer_create", "nus_yuv_resizer_destroy", "nus_yuv_resizer_last_error", "nus_yuv_resizer_set_device",
       "nus_yuv_resizer_initialize", "nus_yuv_resizer_export_axis", "nus_yuv420_resize_device", "nus_yuv420_resize")
CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")
FILTERS = ((0, "lanczos3", 2), (1, "bicubic", 3), (2, "triangle", 4))  # oracle filter, Python name, nus_algorithm
AXES = ((8, 16), (11, 33), (36, 54), (30, 40), (130, 260), (540, 1080), (64, 77), (5, 20))
W_BOUND = 2e-6  # absolute, on weights that sum to 1: numpy's sin rounded to f32 and libm's sinf differ in the last bit


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


@pytest.fixture()
def handle(lib):
    h = lib.nus_yuv_resizer_create()
    assert h
    yield h
    lib.nus_yuv_resizer_destroy(h)


def test_exports_header_and_abi(nsc, lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in nsc._capi.SIGNATURES), name
    raw = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    assert "#define NUS_ABI_VERSION 1\n" in raw and raw.count("NUS_ABI_VERSION") == 1
    assert lib.nus_abi_version() == 1
    hdr = " ".join(raw.split())
    for proto in ("typedef struct nus_yuv_resizer nus_yuv_resizer;", "nus_yuv_resizer *nus_yuv_resizer_create(void);",
                  "void nus_yuv_resizer_destroy(nus_yuv_resizer *h);", "const char *nus_yuv_resizer_last_error(const nus_yuv_resizer *h);",
                  "int nus_yuv_resizer_set_device(nus_yuv_resizer *h, int device);",
                  "int nus_yuv_resizer_initialize(nus_yuv_resizer *h, uint32_t iw, uint32_t ih, uint32_t ow, uint32_t oh, int algorithm, int siting, int mode);",
                  "int nus_yuv_resizer_export_axis(const nus_yuv_resizer *h, int plane, int axis, int32_t *left, uint32_t *ntaps, float *weights);",
                  "int nus_yuv420_resize_device(nus_yuv_resizer *h, const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride, "
                  "uint32_t n_frames, void *stream);",
                  "int nus_yuv420_resize(nus_yuv_resizer *h, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);"):
        assert proto in hdr, proto
    # the new section stands behind the conversions' and is marked as this build's own
    sec = hdr[hdr.index("Up-scaling I420 frames plane by plane"):]
    assert hdr.index("Up-scaling I420 frames plane by plane") > hdr.index("int nus_rgba8_to_yuv420(int device")
    assert "BUILD-DEFINED" in sec[:sec.index("typedef struct nus_yuv_resizer")]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "nus_k_yuv_resize.hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0]
    assert "nus_yuv_resize.cpp" in mk.split("HOST", 1)[1].split("\n", 1)[0]
    head = open(os.path.join(CSRC, "nus_k_yuv_resize.hip")).read().split("#include", 1)[0]
    assert "BUILD-DEFINED" in head and "no scratch" in head and "LDS per workgroup" in head


def test_initialize_checks_its_arguments(nsc, lib, handle):
    C = nsc._capi
    name = "nus_yuv_resizer_initialize"

    def refused(status, text, iw=16, ih=8, ow=32, oh=16, alg=C.ALG_LANCZOS3, siting=0, mode=0, h=handle):
        assert lib.nus_yuv_resizer_initialize(h, iw, ih, ow, oh, alg, siting, mode) == status, text
        msg = C.last_error()
        assert msg.startswith(name + ": ") and text in msg, msg
        if h:
            assert lib.nus_yuv_resizer_last_error(h).decode() == msg

    refused(C.ERR_INVALID_ARGUMENT, "null handle", h=None)
    for kw in (dict(iw=0), dict(ih=0), dict(ow=0), dict(oh=0)):
        refused(C.ERR_INVALID_ARGUMENT, "width and height must be non-zero", **kw)
    refused(C.ERR_INVALID_ARGUMENT, "too large", iw=1 << 16, ih=1 << 15, ow=1 << 16, oh=1 << 15)
    refused(C.ERR_INVALID_ARGUMENT, "output height above 262140", iw=2, ih=2, ow=2, oh=262142)
    for kw in (dict(iw=15), dict(ih=7), dict(ow=33), dict(oh=17)):  # odd sizes
        refused(C.ERR_UNSUPPORTED, "all four dimensions must be even", **kw)
    for kw in (dict(ow=14), dict(oh=6), dict(iw=64, ow=32, oh=16)):  # down-scaling on an axis
        refused(C.ERR_UNSUPPORTED, "down-scaling on an axis is not supported", **kw)
    for text in ("all four dimensions must be even", "down-scaling"):  # the rule is named and the caller pointed to the RGBA route
        kw = dict(iw=15) if "even" in text else dict(ow=14)
        lib.nus_yuv_resizer_initialize(handle, kw.get("iw", 16), 8, kw.get("ow", 32), 16, C.ALG_LANCZOS3, 0, 0)
        assert "RGBA route" in C.last_error() and "nus_upscaler" in C.last_error()
    for alg in (C.ALG_NEAREST, C.ALG_BILINEAR, C.ALG_FSR1, C.ALG_FSR_EASU, C.ALG_FSR_RCAS, 8, -1):
        refused(C.ERR_UNSUPPORTED, f"algorithm {alg} is not supported", alg=alg)
    refused(C.ERR_INVALID_ARGUMENT, "unknown siting 2", siting=2)
    refused(C.ERR_INVALID_ARGUMENT, "unknown siting -1", siting=-1)
    refused(C.ERR_INVALID_ARGUMENT, "unknown mode 2", mode=2)
    refused(C.ERR_INVALID_ARGUMENT, "unknown mode -1", mode=-1)
    for alg in (C.ALG_LANCZOS3, C.ALG_BICUBIC, C.ALG_TRIANGLE):
        for siting in (0, 1):
            for mode in (0, 1):
                assert lib.nus_yuv_resizer_initialize(handle, 16, 8, 32, 16, alg, siting, mode) == C.OK
    assert lib.nus_yuv_resizer_initialize(handle, 16, 8, 16, 8, C.ALG_LANCZOS3, 0, 0) == C.OK  # equal sizes: a copy
    assert lib.nus_yuv_resizer_set_device(handle, -1) == C.ERR_INVALID_ARGUMENT
    assert C.last_error() == "nus_yuv_resizer_set_device: negative device index"
    assert lib.nus_yuv_resizer_set_device(None, 0) == C.ERR_INVALID_ARGUMENT and C.last_error() == "nus_yuv_resizer_set_device: null handle"
    assert lib.nus_yuv_resizer_last_error(None) == b"null handle"


def test_device_entry_point_checks_its_arguments_before_any_hip_call(nsc, lib, handle):
    C = nsc._capi
    name = "nus_yuv420_resize_device"
    IN, OUT = 0x10000, 0x20000  # never dereferenced: every call below is refused first
    in_b, out_b = 16 * 8 * 3 // 2, 32 * 16 * 3 // 2

    def refused(status, text, h=handle, d_in=IN, si=0, d_out=OUT, so=0, n=1):
        assert lib.nus_yuv420_resize_device(h, d_in, si, d_out, so, n, None) == status, text
        msg = C.last_error()
        assert msg.startswith(name + ": ") and text in msg, msg

    refused(C.ERR_INVALID_ARGUMENT, "null handle", h=None)
    refused(C.ERR_NOT_INITIALIZED, "not initialized")
    assert lib.nus_yuv_resizer_initialize(handle, 16, 8, 32, 16, C.ALG_LANCZOS3, 1, 0) == C.OK
    refused(C.ERR_INVALID_ARGUMENT, "null pointer", d_in=None)
    refused(C.ERR_INVALID_ARGUMENT, "null pointer", d_out=None)
    refused(C.ERR_INVALID_ARGUMENT, "n_frames must be at least 1", n=0)
    refused(C.ERR_INVALID_ARGUMENT, f"in_frame_stride must be 0 or at least {in_b}, got {in_b - 1}", si=in_b - 1)
    refused(C.ERR_INVALID_ARGUMENT, f"out_frame_stride must be 0 or at least {out_b}, got {out_b - 1}", so=out_b - 1)
    if C.device_count() == 0:  # odd bases and strides are strides: these pass every check and stop at the device
        for kw in (dict(d_in=IN + 1), dict(si=in_b + 1, n=2), dict(so=out_b + 3, n=2)):
            refused(C.ERR_NO_DEVICE, "no HIP device available", **kw)
    # the Python wrapper maps the statuses as the module's other functions do
    r = nsc.yuv.YuvResizer(16, 8, 32, 16)
    with pytest.raises(ValueError, match=name + ": null pointer"):
        r.resize_device(0, OUT)
    with pytest.raises(ValueError, match="n_frames must be at least 1"):
        r.resize_device(IN, OUT, n_frames=0)
    with pytest.raises(ValueError, match=f"out_frame_stride must be 0 or at least {out_b}"):
        r.resize_device(IN, OUT, out_frame_stride=8)


def test_host_entry_point_checks_its_arguments_before_any_hip_call(nsc, lib, handle):
    C = nsc._capi
    name = "nus_yuv420_resize"
    in_b, out_b = 16 * 8 * 3 // 2, 32 * 16 * 3 // 2
    src, dst = (ctypes.c_ubyte * (in_b + 1))(), (ctypes.c_ubyte * out_b)()

    def refused(status, text, h=handle, s=ctypes.addressof(src), sl=in_b, d=ctypes.addressof(dst), cap=out_b):
        assert lib.nus_yuv420_resize(h, s, sl, d, cap) == status, text
        msg = C.last_error()
        assert msg.startswith(name + ": ") and text in msg, msg

    refused(C.ERR_INVALID_ARGUMENT, "null handle", h=None)
    refused(C.ERR_NOT_INITIALIZED, "not initialized")
    assert lib.nus_yuv_resizer_initialize(handle, 16, 8, 32, 16, C.ALG_BICUBIC, 0, 1) == C.OK
    refused(C.ERR_INVALID_ARGUMENT, "null pointer", s=None)
    refused(C.ERR_INVALID_ARGUMENT, "null pointer", d=None)
    refused(C.ERR_SIZE_MISMATCH, f"in_len ({in_b - 1}) does not match the frame size ({in_b} for 16x8)", sl=in_b - 1)
    refused(C.ERR_SIZE_MISMATCH, f"in_len ({in_b + 1}) does not match the frame size ({in_b} for 16x8)", sl=in_b + 1)
    refused(C.ERR_SIZE_MISMATCH, f"out_cap ({out_b - 1}) is below the frame size ({out_b} for 32x16)", cap=out_b - 1)
    if C.device_count() == 0:
        refused(C.ERR_NO_DEVICE, "no HIP device available")
    r = nsc.yuv.YuvResizer(16, 8, 32, 16)
    with pytest.raises(ValueError, match=name + ": in_len"):
        r.resize(bytes(in_b - 1))


def test_export_axis_checks_its_arguments(nsc, lib, handle):
    C = nsc._capi
    name = "nus_yuv_resizer_export_axis"
    left, ntaps, w = np.zeros(32, np.int32), np.zeros(32, np.uint32), np.zeros((32, 32), np.float32)

    def refused(status, text, h=handle, plane=0, axis=0, a=left.ctypes.data, b=ntaps.ctypes.data, c=w.ctypes.data):
        assert lib.nus_yuv_resizer_export_axis(h, plane, axis, a, b, c) == status, text
        msg = C.last_error()
        assert msg.startswith(name + ": ") and text in msg, msg

    refused(C.ERR_INVALID_ARGUMENT, "null handle", h=None)
    refused(C.ERR_NOT_INITIALIZED, "not initialized")
    assert lib.nus_yuv_resizer_initialize(handle, 16, 8, 32, 16, C.ALG_LANCZOS3, 0, 0) == C.OK
    for kw in (dict(a=None), dict(b=None), dict(c=None)):
        refused(C.ERR_INVALID_ARGUMENT, "null pointer", **kw)
    refused(C.ERR_INVALID_ARGUMENT, "unknown plane 2", plane=2)
    refused(C.ERR_INVALID_ARGUMENT, "unknown axis -1", axis=-1)
    assert lib.nus_yuv_resizer_export_axis(handle, 0, 0, left.ctypes.data, ntaps.ctypes.data, w.ctypes.data) == C.OK
    with pytest.raises(ValueError, match="plane and axis"):
        nsc.yuv.YuvResizer(16, 8, 32, 16).export_axis(2, 0)


def test_python_constructor_maps_its_errors(nsc):
    for kw, text in ((dict(algorithm="spline"), "algorithm"), (dict(siting="top"), "siting"), (dict(mode="fast"), "mode")):
        with pytest.raises(ValueError, match=text):
            nsc.yuv.YuvResizer(16, 8, 32, 16, **kw)
    for alg in ("nearest", "bilinear", "fsr1"):
        with pytest.raises(RuntimeError, match="nus_yuv_resizer_initialize: algorithm . is not supported"):
            nsc.yuv.YuvResizer(16, 8, 32, 16, algorithm=alg)
    with pytest.raises(RuntimeError, match="all four dimensions must be even"):
        nsc.yuv.YuvResizer(15, 8, 30, 16)
    with pytest.raises(RuntimeError, match="down-scaling"):
        nsc.yuv.YuvResizer(16, 8, 8, 16)
    with pytest.raises(ValueError, match="width and height must be non-zero"):
        nsc.yuv.YuvResizer(0, 8, 32, 16)
    r = nsc.yuv.YuvResizer(16, 8, 32, 16, "catmullrom", "left", "exact")
    assert (r.in_frame_bytes, r.out_frame_bytes) == (192, 768)


@pytest.mark.parametrize("filt,alg,_", FILTERS)
def test_exported_axes_are_the_oracles_and_the_restatements(nsc, oracle_mod, filt, alg, _):
    """Luma x and y, chroma y and, under centre siting, chroma x: oracle.resize_axis' windows exactly, its weights within 2e-6.
    Chroma x under left siting: the same against _plane_resample64.axis(.., 0.25).  Worst weight difference seen here: 0 against
    the oracle (the tables are bit-equal), 1.2e-7 against the restatement."""
    worst = {"oracle": 0.0, "restatement": 0.0}
    for iw, ih, ow, oh in ((16, 8, 32, 16), (22, 10, 66, 30), (64, 36, 96, 54), (60, 80, 80, 120), (260, 12, 520, 12), (10, 1080, 40, 2160)):
        for siting in ("center", "left"):
            r = nsc.yuv.YuvResizer(iw, ih, ow, oh, alg, siting)
            for plane in (0, 1):
                for ax in (0, 1):
                    left, ntaps, w = r.export_axis(plane, ax)
                    i_n, o_n = ((iw, ih)[ax]) // (1 + plane), ((ow, oh)[ax]) // (1 + plane)
                    if plane == 1 and ax == 0 and siting == "left":
                        L, N, W = P.axis(i_n, o_n, filt, 0.25)
                        key = "restatement"
                    else:
                        L, N, W = oracle_mod.resize_axis(i_n, o_n, filt)
                        key = "oracle"
                    tag = f"{alg} {iw}x{ih}->{ow}x{oh} {siting} plane {plane} axis {ax}"
                    np.testing.assert_array_equal(left, L, err_msg=tag)
                    np.testing.assert_array_equal(ntaps, N, err_msg=tag)
                    d = float(np.abs(w.astype(np.float64) - np.asarray(W, np.float64)).max())
                    worst[key] = max(worst[key], d)
                    assert d <= W_BOUND, (tag, d)
                    assert int(ntaps.max()) <= 8, tag  # the dimension rule's tap bound
                    assert (w[np.arange(32)[None, :] >= ntaps[:, None]] == 0).all(), tag  # zero padded
    print(f"worst weight difference ({alg}): {worst}")
    # left siting moves the chroma x axis: it is not the centre-sited table
    a = nsc.yuv.YuvResizer(64, 36, 96, 54, alg, "left").export_axis(1, 0)
    b = nsc.yuv.YuvResizer(64, 36, 96, 54, alg, "center").export_axis(1, 0)
    assert float(np.abs(a[2] - b[2]).max()) > 1e-3


@pytest.mark.parametrize("filt,alg,_", FILTERS)
def test_restatement_reproduces_the_oracles_windows(oracle_mod, filt, alg, _):
    """At phi = 0.5 the numpy restatement gives oracle.resize_axis' left and ntaps exactly and its weights within 2e-6 (8.3e-7 when
    first measured; 1.2e-7 here)."""
    worst = 0.0
    for i_n, o_n in AXES:
        left, ntaps, w = oracle_mod.resize_axis(i_n, o_n, filt)
        L, N, W = P.axis(i_n, o_n, filt, 0.5)
        np.testing.assert_array_equal(left, L, err_msg=f"{alg} {i_n}->{o_n}")
        np.testing.assert_array_equal(ntaps, N, err_msg=f"{alg} {i_n}->{o_n}")
        worst = max(worst, float(np.abs(np.asarray(w, np.float64) - W).max()))
    print(f"worst weight difference ({alg}): {worst}")
    assert worst <= W_BOUND
    # phi = 0.25 on a x2 axis: output o sits at (o + 0.25) / 2 + 0.25 - 0.5 input samples: output 0 on input sample 0 - 1/8
    L, N, W = P.axis(8, 16, 2, 0.25)  # triangle: two taps, linear in the distance
    c =(4 + 0.25) * 0.5 + 0.25 - 0.5  # 1.875: between samples 1 and 2
    got = sum(float(W[4, k]) * (L[4] + k) for k in range(int(N[4])))
    assert abs(got - c) < 1e-6


SCAN_IN = range(4, 1101, 4)  # every row-form-eligible input width of an x axis, and below every output width in [in, 4 in]
SCAN_API_IN = tuple(range(4, 1101, 48)) + (1100,)  # the part of it that goes through the library: 24 input widths ...


def _scan_api_out(in_n):  # ... each with the ten ratios closest to 1 and every eleventh output width above them
    return sorted(set(range(in_n, min(in_n + 40, 4 * in_n + 1), 4)) | set(range(in_n, 4 * in_n + 1, 44)))


@pytest.mark.parametrize("filt,alg,_", FILTERS)
def test_no_row_form_axis_needs_the_12_wide_union(nsc, filt, alg, _):
    """Which k_plane_rows instance can a public call reach?  Every x axis that the row form takes (both widths multiples of 4) for
    input widths 4 .. 1100 and output widths in .. 4 in, both sample positions: the widest tap window and the widest union of the
    windows of a lane's four outputs (row_geometry: the loop of YuvResizer::initialize).  114 125 axes per filter and position
    come from _plane_resample64.windows, the float32 restatement of the window expressions; 1 133 of them (SCAN_API_IN x
    _scan_api_out) are also built by the library, as the chroma x axis of a 2 in x 2 -> 2 out x 2 handle under either siting, and
    must give the restatement's windows exactly.  Found: Lanczos-3 7 taps and union 10, Catmull-Rom 5 and 8, Triangle 3 and 6,
    the same at 0.5 and 0.25, all reached at ratio 1 (8 -> 8, 12 -> 12).  So launch_plane_resize's `union_taps <= 10` always
    holds in this range and k_plane_rows<*, 12> is never launched."""
    expected = {0: (7, 10), 1: (5, 8), 2: (3, 6)}[filt]
    axes = checked = 0
    for phi, siting in ((0.5, "center"), (0.25, "left")):
        taps = union = 0
        for in_n in SCAN_IN:
            outs = np.arange(in_n, 4 * in_n + 1, 4)
            for c in range(0, len(outs), 48):  # (blocks that stay in the cache)
                lo, n, valid = P.windows(in_n, outs[c:c + 48], filt, phi)
                end = lo + n
                un = (end.reshape(len(end), -1, 4).max(axis=2) - lo[:, ::4])[valid[:, ::4]]
                assert (n[valid] >= 1).all() and (un >= 1).all()
                taps, union = max(taps, int(n.max())), max(union, int(un.max()))
            axes += len(outs)
            if in_n in SCAN_API_IN:
                for out_n in _scan_api_out(in_n):
                    left, ntaps, _w = nsc.yuv.YuvResizer(2 * in_n, 2, 2 * out_n, 2, alg, siting).export_axis(1, 0)
                    lo, n, _v = P.windows(in_n, [out_n], filt, phi)
                    np.testing.assert_array_equal(left, lo[0], err_msg=f"{alg} {in_n}->{out_n} {siting}")
                    np.testing.assert_array_equal(ntaps, n[0], err_msg=f"{alg} {in_n}->{out_n} {siting}")
                    u = P.row_geometry(left, ntaps, out_n)[1]
                    assert u == int(((lo[0] + n[0]).reshape(-1, 4).max(axis=1) - lo[0, ::4]).max())
                    assert u <= expected[1]
                    checked += 1
        print(f"{alg} phi {phi}: most taps {taps}, widest union {union}")
        assert taps <= 7 and union <= 10, (alg, phi, taps, union)  # the bound that makes the 12-wide instance unreachable
        assert (taps, union) == expected, (alg, phi, taps, union)  # and what the scan recorded
    assert axes == 2 * 114125 and checked == 2 * 1133, (axes, checked)


def test_the_launch_cases_of_the_gpu_tests_are_what_they_say(nsc):
    """tests/test_gpu_yuv_resize_launch.py asserts, before it runs a case, the numbers that make the case one: they need no device,
    so they are held here as well -- the rows per block of the long batches, the footprints and unions of the wide segments, the
    pool frames around the grid-z split, and that each filter's seeded sweep holds at least 4 shapes of every class and form."""
    import test_gpu_yuv_resize_launch as L

    assert [(L._rpb(32, 40, n), L._rpb(16, 20, 2 * n)) for n in (5, 1000, 2000, 3400)] == [(8, 8), (9, 9), (19, 19), (32, 32)]
    assert L._row_blocks(40, 9) == [9, 9, 9, 9, 4] and L._row_blocks(20, 19) == [19, 1] and L._row_blocks(20, 32) == [20]
    assert L._rpb(3840, 2160, 31) == 32 and L._rpb(1920, 1080, 62) == 32  # the measured workload: 31 frames, 1080p -> 4K
    for shape, luma, chroma in L.WIDE:
        L._assert_wide_case(nsc, shape, luma, chroma)
    for alg in ("bicubic", "triangle"):
        L._assert_wide_case(nsc, (520, 8, 520, 16), (">256", None), (">256", None), alg)
    assert L._geometry(nsc, (1016, 8, 1024, 16), "lanczos3", "left") == ((264, 10), (260, 10))
    assert L._geometry(nsc, (504, 8, 512, 16), "lanczos3", "center") == ((256, 10), (252, 10))
    widest = max(max(g[0] for g in L._geometry(nsc, s, "lanczos3", "left")) for s in L.T.FIRST + L.T.REST if s[:2] != s[2:])
    assert widest == 72  # what tests/test_gpu_yuv_resize.py reaches: one sweep of the V pass everywhere
    L._pool(8, 4, 32769, 1, L.SPLIT_RESIZE)
    L._pool(4, 2, 65537, 1, L.SPLIT_COPY)
    assert len(set(L.SWEEP_SEEDS.values())) == 3
    for alg in L.SWEEP_SEEDS:
        shapes = L.sweep_shapes(alg)
        forms = L.sweep_forms(shapes)
        print(alg, forms)
        assert len(shapes) == 20 and len(set(shapes)) == 20 and min(forms.values()) >= 4, (alg, forms)


def test_plane_witness_on_a_ramp(oracle_mod):
    """The float64 witness with the triangle filter (linear interpolation on an up-scale) maps a horizontal ramp onto itself away
    from the borders, at the position the siting gives: under phi = 0.25 output o of a x2 axis reads (o + 0.25) / 2 - 0.25."""
    iw, ih = 32, 6
    plane = np.tile((np.arange(iw) * 4).astype(np.uint8), (ih, 1))
    for phi, pos in ((0.5, lambda o: (o + 0.5) / 2 - 0.5), (0.25, lambda o: (o + 0.25) / 2 - 0.25)):
        v = P.plane_resample64(oracle_mod, plane, 64, 12, 2, phi)
        o = np.arange(16, 48)
        np.testing.assert_allclose(v[5, 16:48], 4 * pos(o), atol=1e-4)
    np.testing.assert_array_equal(P.plane_resample64(oracle_mod, plane, iw, ih, 0, 0.25), plane.astype(np.float64))


def test_scale_domain_refusals(nsc, tmp_path):
    from nu_scaler_amd.video import check_convert_args, convert_y4m, default_window_frames, window_bytes_per_frame
    from nu_scaler_amd.y4m import Y4MWriter

    ok = check_convert_args(24, 60, None, "blend", 2, False, scale_domain="yuv", algorithm="lanczos3", width=64, height=48)
    assert ok[1:] == (5, 2)
    assert check_convert_args(24, 60, None, "blend", 2, False) == ok  # the keyword's default is today's route
    with pytest.raises(ValueError, match="scale_domain must be 'rgb' or 'yuv'"):
        check_convert_args(24, 60, None, "blend", 2, False, scale_domain="ycbcr")
    for alg in ("nearest", "bilinear", "fsr1", "fsr", "easu", "rcas"):
        with pytest.raises(ValueError, match="scale_domain 'yuv' resamples the Y, U and V planes with lanczos3, bicubic or triangle"):
            check_convert_args(24, 60, None, "blend", 2, False, scale_domain="yuv", algorithm=alg)
        check_convert_args(24, 60, None, "blend", 2, False, scale_domain="rgb", algorithm=alg)
    for kw in (dict(width=63, height=48), dict(width=64, height=47)):
        with pytest.raises(ValueError, match="scale_domain 'yuv' needs an even width and height"):
            check_convert_args(24, 60, None, "blend", 2, False, scale_domain="yuv", **kw)
        check_convert_args(24, 60, None, "blend", 2, False, scale_domain="rgb", **kw)
    # convert_y4m raises them from the file's header, before any device work
    src = str(tmp_path / "odd.y4m")
    with Y4MWriter(src, 63, 48, 24, "center") as wr:
        for _ in range(2):
            wr.write(bytes(63 * 48 + 2 * 32 * 24))
    with pytest.raises(ValueError, match="needs an even width and height"):
        convert_y4m(src, str(tmp_path / "o.y4m"), fps_out=60, method="blend", scale=2, scale_domain="yuv")
    with pytest.raises(ValueError, match="scale_domain must be"):
        convert_y4m(src, str(tmp_path / "o.y4m"), fps_out=60, method="blend", scale=2, scale_domain="planar")
    with pytest.raises(ValueError, match="not with 'bilinear'"):
        convert_y4m(src, str(tmp_path / "o.y4m"), fps_out=60, method="blend", scale=2, algorithm="bilinear", scale_domain="yuv")
    # the window sizes: the five-argument values stay; the planar route holds no target-size RGBA
    w, h = 1920, 1080
    yuv_in, rgba_in, yuv_out = w * h * 3 // 2, w * h * 4, 4 * w * h * 3 // 2
    assert window_bytes_per_frame(w, h, 5, 2, 2) == window_bytes_per_frame(w, h, 5, 2, 2, "rgb")
    assert window_bytes_per_frame(w, h, 5, 2, 2, "yuv") == yuv_in + rgba_in + -(-(rgba_in + yuv_in + yuv_out) * 5 // 2)
    assert window_bytes_per_frame(w, h, 1, 1, 2, "yuv") == yuv_in + yuv_out
    assert window_bytes_per_frame(w, h, 5, 2, 1, "yuv") == window_bytes_per_frame(w, h, 5, 2, 1)
    assert window_bytes_per_frame(w, h, 5, 2, 2, "yuv") < window_bytes_per_frame(w, h, 5, 2, 2)
    assert callable(default_window_frames)


def test_cli_flag(nsc, capsys):
    from nu_scaler_amd import cli

    p = cli.build_parser()
    a = p.parse_args(["video", "in.y4m", "out.y4m", "--to", "60", "--scale", "2", "--scale-domain", "yuv"])
    assert a.scale_domain == "yuv"
    assert p.parse_args(["video", "in.y4m", "out.y4m", "--to", "60"]).scale_domain == "rgb"
    with pytest.raises(SystemExit) as e:
        p.parse_args(["video", "in.y4m", "out.y4m", "--to", "60", "--scale-domain", "ycc"])
    assert e.value.code == 2
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        p.parse_args(["video", "--help"])
    assert e.value.code == 0
    assert "--scale-domain" in capsys.readouterr().out
