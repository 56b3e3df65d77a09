"""The planar up-scaler at the launch shapes of the real workload (nus_k_yuv_resize.hip: launch_plane_resize, k_plane_rows,
k_frame_copy), which the small frames and batches of test_gpu_yuv_resize.py never reach.  Every test first asserts, from the
launcher's own numbers, that its case is what it says -- the rows per block, the segment footprint, the union, the chunk count,
the form -- and then holds the bytes to what test_gpu_yuv_resize.py holds them to: the float64 witness of
tests/_plane_resample64.py under _resample64.assert_fma_contract, or the same entry point's result on a short batch which the
witness holds.
  rows per block      rpb = clamp(oh * blocks_x * planes / 4096, 8, 32): 9, 19 and 32 by the batch length, with a last block that
                      is shorter, and a block longer than the plane.  The union weights and the zeroed LDS slack are set up once
                      before the row loop; the fences between a row's H pass and the next row's V pass order the LDS row's reuse.
  wide segments       an input footprint above 256 columns gives the V pass a second sweep; ratios between 1 and 1.5 give a lane's
                      run left-edge shifts of 0 .. 3 and the widest unions (10; see test_yuv_resize_host.py for the bound).
  the grid-z split    for_grid_z_chunks cuts at 65535 planes, an odd number: the chroma launch's second chunk starts at the V plane
                      of frame 32767, the copy's at frame 65535.
  a seeded sweep      20 shapes per filter, every class in both forms."""
import os

import numpy as np
import pytest

import _plane_resample64 as P
import _resample64 as R
import test_gpu_yuv_resize as T
from conftest import ROOT

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")
MAX_GRID_Z = 65535
_cache = {}


# ---------------------------------------------------------------- the launcher's numbers, restated

def _launcher_source():
    if "src" not in _cache:
        _cache["src"] = (open(os.path.join(CSRC, "nus_k_yuv_resize.hip")).read(), open(os.path.join(CSRC, "nus_device.hpp")).read(),
                         open(os.path.join(CSRC, "nus_kernels.hpp")).read())
    return _cache["src"]


def _rpb(ow, oh, planes):
    """rows_per_block of a row-form launch of `planes` planes (one grid-z chunk), as launch_plane_resize computes it.  The
    formula's text is asserted, so that a change to it fails here and has to be restated."""
    unit, device, kernels = _launcher_source()
    assert "const uint64_t blocks_x = cdiv(cdiv(L.ow, kPlaneSegment), 4);" in unit
    assert "uint64_t rpb = (uint64_t)L.oh * blocks_x * n / 4096;" in unit
    assert "rpb = rpb < 8 ? 8 : (rpb > 32 ? 32 : rpb);" in unit
    assert "const dim3 grid((uint32_t)blocks_x, cdiv(L.oh, (uint32_t)rpb), n);" in unit
    assert "constexpr uint32_t kPlaneRun = 4;" in kernels and "constexpr uint32_t kPlaneSegment = 64 * kPlaneRun;" in kernels
    assert f"constexpr uint32_t kMaxGridZ = {MAX_GRID_Z};" in device
    assert planes <= MAX_GRID_Z
    blocks_x = -(-(-(-ow // 256)) // 4)
    return min(max(oh * blocks_x * planes // 4096, 8), 32)


def _row_blocks(oh, rpb):
    return [min(rpb, oh - y) for y in range(0, oh, rpb)]


def _rows_form(in_w, out_w):
    """plane_rows_form for a plane class of a tight, dword-aligned batch of even-sized frames: the widths decide (every plane
    offset, plane step and frame stride is then a multiple of 4, and no window of an up-scale exceeds 8 taps)."""
    return in_w % 4 == 0 and out_w % 4 == 0


def _geometry(nsc, shape, alg, siting):
    """((ncols_max, union) of luma, of chroma) from the exported x axes, by the two loops of YuvResizer::initialize; (0, 0) for a
    class that the row form does not take."""
    iw, ih, ow, oh = shape
    r = nsc.yuv.YuvResizer(iw, ih, ow, oh, alg, siting)
    out = []
    for plane, n in ((0, ow), (1, ow // 2)):
        left, ntaps, _ = r.export_axis(plane, 0)
        assert int(ntaps.max()) <= 8
        out.append(P.row_geometry(left, ntaps, n) if _rows_form(iw >> plane, n) else (0, 0))
    return tuple(out)


def _witness(oracle_mod, src, shape, alg, siting):
    """T._witness for frames of this module's own: per frame of `src` the float64 planes (Y, U, V), and the eps per plane class."""
    iw, ih, ow, oh = shape
    filt = T.FILTERS[alg]
    phi = 0.25 if siting == "left" else 0.5
    v = []
    for fr in src:
        y, u, c = T._split(fr, iw, ih)
        v.append((P.plane_resample64(oracle_mod, y, ow, oh, filt, 0.5), P.plane_resample64(oracle_mod, u, ow // 2, oh // 2, filt, phi),
                  P.plane_resample64(oracle_mod, c, ow // 2, oh // 2, filt, phi)))
    return v, (P.plane_eps(oracle_mod, iw, ih, ow, oh, filt, 0.5), P.plane_eps(oracle_mod, iw // 2, ih // 2, ow // 2, oh // 2, filt, phi))


def _hold(got, witness, shape, tag):
    """Every plane of every frame of `got` inside the contract, as T._check holds them."""
    v, eps = witness
    assert len(got) == len(v)
    for k in range(len(got)):
        for name, g, want, e in zip("YUV", T._split(got[k], *shape[2:]), v[k], (eps[0], eps[1], eps[1])):
            R.assert_fma_contract(g[..., None], want[..., None], e, f"{tag} frame {k} plane {name}")


# ---------------------------------------------------------------- long batches: more than 8 rows per block

LONG = (16, 20, 32, 40)


@pytest.mark.parametrize("mode", ("fma", "exact"))
@pytest.mark.parametrize("n,rpb,luma_blocks,chroma_blocks", ((1000, 9, [9, 9, 9, 9, 4], [9, 9, 2]), (2000, 19, [19, 19, 2], [19, 1]),
                                                             (3400, 32, [32, 8], [20])))
def test_long_batches_run_more_than_8_rows_per_block(nsc, n, rpb, luma_blocks, chroma_blocks, mode):
    """The five content frames cycled to n frames give the 5-frame call's bytes, cycled; test_gpu_yuv_resize.py holds the 5-frame
    call of this shape to the witness and the oracle.  n = 2000 runs with padded strides as well (the gaps keep their poison: _run)."""
    iw, ih, ow, oh = LONG
    assert _rows_form(iw, ow) and _rows_form(iw // 2, ow // 2)
    assert _rpb(ow, oh, n) == rpb and _row_blocks(oh, rpb) == luma_blocks
    assert _rpb(ow // 2, oh // 2, 2 * n) == rpb and _row_blocks(oh // 2, rpb) == chroma_blocks
    assert 2 * n <= MAX_GRID_Z  # one launch per class: the whole batch counts in the formula
    assert _rpb(ow, oh, 5) == 8 and _rpb(ow // 2, oh // 2, 10) == 8  # (the 5-frame call is the old case)
    base = T._frames(iw, ih)
    pick = np.arange(n) % len(base)
    for siting in ("center", "left"):
        five = T._run(nsc, base, LONG, "lanczos3", siting, mode)
        got = T._run(nsc, base[pick], LONG, "lanczos3", siting, mode)
        np.testing.assert_array_equal(got, five[pick], err_msg=f"{n} frames {siting} {mode}")
        if n == 2000:
            got = T._run(nsc, base[pick], LONG, "lanczos3", siting, mode, in_gap=24, out_gap=40)
            np.testing.assert_array_equal(got, five[pick], err_msg=f"{n} frames {siting} {mode}, padded strides")


# ---------------------------------------------------------------- wide segments, ratios close to 1

#        shape                  luma: ncols_max, union     chroma: ncols_max, union      (None: not what the case is about)
WIDE = (((1016, 8, 1024, 16), (">256", None), (">256", None)),  # footprints of 264 / 260: a second sweep with a few lanes
        ((504, 8, 512, 16), ("==256", None), (None, None)),      # exactly 256: one sweep, every lane busy
        ((520, 8, 520, 16), (">256", 10), (">256", 10)),         # x unchanged: 3 luma segments, the last 8 wide; chroma 260 in 2
        ((64, 8, 80, 16), (None, 10), (None, 10)),               # ratio 5/4
        ((40, 8, 48, 16), (None, 10), (None, 10)),               # ratio 6/5
        ((240, 8, 320, 16), (None, None), (None, None)))         # ratio 4/3: 1080p -> 1440p


def _assert_wide_case(nsc, shape, luma, chroma, alg="lanczos3"):
    iw, _, ow, _ = shape
    assert _rows_form(iw, ow) and _rows_form(iw // 2, ow // 2) and 1.0 <= ow / iw < 1.5
    for siting in ("center", "left"):
        for (ncols, union), (want_cols, want_union), name in zip(_geometry(nsc, shape, alg, siting), (luma, chroma), ("luma", "chroma")):
            tag = (shape, siting, name, ncols, union)
            assert ncols % 4 == 0 and union <= 10, tag
            if want_cols == ">256":
                assert 256 < ncols <= 256 + 16, tag  # a second sweep of the V pass: at most four lanes of it busy
            if want_cols == "==256":
                assert ncols == 256, tag
            if want_union is not None and alg == "lanczos3":
                assert union == want_union, tag


@pytest.mark.parametrize("mode", ("fma", "exact"))
@pytest.mark.parametrize("siting", ("center", "left"))
@pytest.mark.parametrize("shape,luma,chroma", WIDE)
def test_wide_segments_at_ratios_close_to_1(nsc, oracle_mod, shape, luma, chroma, siting, mode):
    _assert_wide_case(nsc, shape, luma, chroma)
    if shape == (1016, 8, 1024, 16):
        assert _geometry(nsc, shape, "lanczos3", "center") == ((264, 10), (260, 10))  # what the restatement gives for it
    if shape == (520, 8, 520, 16):
        assert (-(-520 // 256), 520 - 2 * 256, -(-260 // 256)) == (3, 8, 2)
    T._check(nsc, oracle_mod, shape, "lanczos3", siting, mode)


@pytest.mark.parametrize("mode", ("fma", "exact"))
@pytest.mark.parametrize("siting", ("center", "left"))
@pytest.mark.parametrize("alg", ("bicubic", "triangle"))
def test_an_unchanged_x_axis_with_the_other_filters(nsc, oracle_mod, alg, siting, mode):
    shape = (520, 8, 520, 16)
    _assert_wide_case(nsc, shape, (">256", None), (">256", None), alg)
    T._check(nsc, oracle_mod, shape, alg, siting, mode)


# ---------------------------------------------------------------- the grid-z split

SPLIT_RESIZE = (32766, 32767, 32768)  # the frames around the chroma launch's split: z0 = 65535 is the V plane of frame 32767
SPLIT_COPY = (65534, 65535, 65536)    # and around the copy's


def _pool(w, h, n, seed, around):
    """(7 distinct random frames with U != V, a seeded index array [n] whose entries around the split differ pairwise)."""
    key = ("pool", w, h, n, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        pool = rng.integers(0, 256, (7, T._nbytes(w, h)), dtype=np.uint8)
        idx = rng.integers(0, 7, n)
        assert len({p.tobytes() for p in pool}) == 7
        for p in pool:
            _, u, v = T._split(p, w, h)
            assert (u != v).any()
        assert len({int(idx[k]) for k in around}) == len(around), [int(idx[k]) for k in around]
        pool.setflags(write=False)
        _cache[key] = (pool, idx)
    return _cache[key]


@pytest.mark.parametrize("mode", ("fma", "exact"))
def test_the_chroma_launch_crosses_the_grid_z_split(nsc, oracle_mod, mode):
    """32769 frames of 8x4 -> 16x8: the luma launch is one chunk of 32769 planes, the chroma launch 65538 planes in two chunks, the
    second of which starts at plane 65535 = the V plane of frame 32767 (z0 odd: z / 2 and z % 2 with an odd base).  Row form, then
    -- bases offset by one byte -- the per-sample form.  Every frame is one of 7 pool frames, whose results the witness holds."""
    shape, n = (8, 4, 16, 8), 32769
    assert _rows_form(8, 16) and _rows_form(4, 8)
    chunks = lambda planes: [min(MAX_GRID_Z, planes - d) for d in range(0, planes, MAX_GRID_Z)]  # noqa: E731
    assert chunks(n) == [n] and chunks(2 * n) == [MAX_GRID_Z, 3]
    assert (MAX_GRID_Z // 2, MAX_GRID_Z % 2) == (32767, 1)
    assert _rpb(16, 8, n) == 32 and _rpb(8, 4, MAX_GRID_Z) == 32 and _rpb(8, 4, 3) == 8
    pool, idx = _pool(8, 4, n, 1, SPLIT_RESIZE)
    want = T._run(nsc, pool, shape, "lanczos3", "left", mode)
    _hold(want, _witness(oracle_mod, pool, shape, "lanczos3", "left"), shape, f"pool {mode}")
    assert len({w.tobytes() for w in want}) == 7
    got = T._run(nsc, pool[idx], shape, "lanczos3", "left", mode)
    np.testing.assert_array_equal(got, want[idx], err_msg="row form")
    got = T._run(nsc, pool[idx], shape, "lanczos3", "left", mode, in_off=1, out_off=1)
    np.testing.assert_array_equal(got, want[idx], err_msg="per-sample form")


def test_the_copy_crosses_the_grid_z_split(nsc):
    """65537 frames of 4x2 -> 4x2 (12 bytes): k_frame_copy's second chunk starts at frame 65535.  Dwords, then -- bases offset by
    one byte -- bytes."""
    shape, n = (4, 2, 4, 2), 65537
    assert n > MAX_GRID_Z and T._nbytes(4, 2) % 4 == 0
    pool, idx = _pool(4, 2, n, 1, SPLIT_COPY)
    for kw in (dict(), dict(in_off=1, out_off=1)):
        np.testing.assert_array_equal(T._run(nsc, pool[idx], shape, **kw), pool[idx], err_msg=str(kw))


# ---------------------------------------------------------------- a seeded sweep over shapes

SWEEP_SEEDS = {"lanczos3": 31, "bicubic": 60, "triangle": 101}  # chosen so that every class has 4 shapes in either form
SWEEP_AREA = 400000  # output luma samples: keeps the float64 witness of a shape well under a second


def sweep_shapes(alg):
    """20 x (iw, ih, ow, oh, siting): iw, ih even in 4 .. 300, ow, oh even in in .. 4 in, ow <= 1200, ow * oh <= SWEEP_AREA."""
    rng = np.random.default_rng(SWEEP_SEEDS[alg])
    out = []
    for _ in range(20):
        iw, ih = (2 * int(rng.integers(2, 151)) for _ in range(2))
        ow = min(2 * int(rng.integers(iw // 2, 2 * iw + 1)), 1200)
        oh = 2 * int(rng.integers(ih // 2, 2 * ih + 1))
        if ow * oh > SWEEP_AREA:
            oh = max(ih, SWEEP_AREA // ow & ~1)
        if ow * oh > SWEEP_AREA:
            ow = max(iw, SWEEP_AREA // oh & ~1)
        if (ow, oh) == (iw, ih):
            oh += 2  # (equal sizes are the copy)
        out.append((iw, ih, ow, oh, ("center", "left")[int(rng.integers(0, 2))]))
    return out


def sweep_forms(shapes):
    forms = {"luma-rows": 0, "luma-per-sample": 0, "chroma-rows": 0, "chroma-per-sample": 0}
    for iw, ih, ow, oh, _ in shapes:
        forms["luma-rows" if _rows_form(iw, ow) else "luma-per-sample"] += 1
        forms["chroma-rows" if _rows_form(iw // 2, ow // 2) else "chroma-per-sample"] += 1
    return forms


@pytest.mark.parametrize("alg", tuple(T.FILTERS))
def test_a_seeded_sweep_of_shapes(nsc, oracle_mod, alg):
    shapes = sweep_shapes(alg)
    assert len(shapes) == 20
    forms = sweep_forms(shapes)
    assert min(forms.values()) >= 4, forms
    for k, (iw, ih, ow, oh, siting) in enumerate(shapes):
        assert 4 <= iw <= 300 and 4 <= ih <= 300 and iw <= ow <= min(4 * iw, 1200) and ih <= oh <= 4 * ih and ow * oh <= SWEEP_AREA
        assert not (iw | ih | ow | oh) & 1 and (iw, ih) != (ow, oh)
        src = np.random.default_rng(977 * k + T.FILTERS[alg]).integers(0, 256, (2, T._nbytes(iw, ih)), dtype=np.uint8)
        witness = _witness(oracle_mod, src, (iw, ih, ow, oh), alg, siting)
        for mode in ("fma", "exact"):
            got = T._run(nsc, src, (iw, ih, ow, oh), alg, siting, mode)
            _hold(got, witness, (iw, ih, ow, oh), f"sweep {alg} #{k} {iw}x{ih}->{ow}x{oh} {siting} {mode}")
