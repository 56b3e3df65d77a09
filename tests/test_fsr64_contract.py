"""The C oracle's FSR1 passes (orc_fsr_easu / orc_fsr_rcas) against the float64 witness of the two shaders (tests/_fsr64.py), and
the witness's own teeth.  PARITY UNPINNED still: the reference never dispatches the shaders (fsr.rs:24-260), so no vector of its
own exists; what holds FSR1 is this witness -- written from the definitions, sharing no code with the oracle or its numpy twin.

Measured on the case list (single-valued share = decided samples with ONE permitted byte / all samples):
  EASU, noise and gradient   0.998-1.000 at x2, x2.35, x2.57 / x1.87, x26 / x22, x0.91 / x0.83 and x1 on noise; 0.887-0.889 at
                             x3/2 (one sample in nine has fx = fy = 0: a tap at d = 2); 0.590 for the gradient at x1 (v lands on
                             integers).  The floors asserted below, 0.95 and 0.85, keep the test from going blind.
  EASU, flat / edge          0 / 0.05-0.82: v on an integer has two permitted bytes, wx = 0.5 puts taps at d = 2.
  RCAS at 0.7                0.39-1.0 (low after x26, where the EASU image is smooth and v lands near integers); at 0: 1.0 (pinned).
  a 1 x 1 frame              is flat content: two permitted bytes per sample, exempt from the floors like the flat image.
"""
import numpy as np
import pytest

import _fsr64 as F

_f = np.float32
MUTANTS = ("wx_wy_swapped", "mix_reversed", "tap_base_x_minus_2", "vgx_from_left_right", "centre_half_dropped", "dir_constant_0.001")


def _twin(img, ow, oh, sharp, mutant=None):
    """EASU in numpy f32, operation for operation as the oracle (fsr.rs:104-166), with one-edit mutants."""
    ih, iw = img.shape[:2]
    s = _f(sharp)
    gx, gy = np.meshgrid(np.arange(ow), np.arange(oh))
    half = _f(0.0) if mutant == "centre_half_dropped" else _f(0.5)
    cx = (gx.astype(_f) + half) * (_f(iw) / _f(ow))
    cy = (gy.astype(_f) + half) * (_f(ih) / _f(oh))
    ix, iy = cx.astype(np.int32), cy.astype(np.int32)
    fx, fy = cx - np.floor(cx), cy - np.floor(cy)

    def fetch(x, y):
        return img[np.clip(y, 0, ih - 1), np.clip(x, 0, iw - 1), :3].astype(_f) / _f(255.0)

    a, b = np.abs(fetch(ix, iy - 1) - fetch(ix, iy + 1)), np.abs(fetch(ix - 1, iy) - fetch(ix + 1, iy))
    if mutant == "vgx_from_left_right":
        a, b = b, a
    k = _f(0.001) if mutant == "dir_constant_0.001" else _f(0.0001)
    dx, dy = (a[..., 0] + a[..., 1] + a[..., 2]) / _f(3.0) + k, (b[..., 0] + b[..., 1] + b[..., 2]) / _f(3.0) + k
    ln = np.sqrt(dx * dx + dy * dy)
    dx, dy = dx / ln, dy / ln
    wx = np.abs(dx) / (np.abs(dx) + np.abs(dy))
    wy = _f(1.0) - wx
    if mutant == "wx_wy_swapped":
        wx, wy = wy, wx
    base = 2 if mutant == "tap_base_x_minus_2" else 1
    acc, accw = np.zeros((oh, ow, 3), _f), np.zeros((oh, ow), _f)
    for y in range(4):
        for x in range(4):
            d = np.abs((_f(x) - fx) * wx + (_f(y) - fy) * wy)
            d2 = d * d
            d3 = d * d2
            w = np.where(d <= 1, _f(2.0) - _f(1.5) * d - _f(0.5) * d3 + d2,
                         np.where(d <= 2, _f(0.0) - _f(0.5) * d + _f(2.5) * d2 - d3, _f(0.0))).astype(_f)
            acc = acc + fetch(ix - base + x, iy - 1 + y) * w[..., None]
            accw = accw + w
    col = acc / np.maximum(accw, _f(0.0001))[..., None]
    if s > _f(0.001):
        col = col * s + fetch(ix, iy) * (_f(1.0) - s) if mutant == "mix_reversed" else col * (_f(1.0) - s) + fetch(ix, iy) * s
    out = np.full((oh, ow, 4), 255, np.uint8)
    out[..., :3] = (np.minimum(np.maximum(col, _f(0.0)), _f(1.0)) * _f(255.0)).astype(np.uint32)
    return out


@pytest.fixture(scope="module")
def witnessed(oracle_mod):
    """Every EASU case once: {(dims, content, sharpness): (image, Witness)}; computed once, left unchanged."""
    out = {}
    for dims in F.CASES:
        (w, h), (ow, oh) = dims
        for name, img in F.contents(oracle_mod, w, h).items():
            for es in F.EASU_SHARPNESS:
                out[dims, name, es] = (img, F.easu64(img, ow, oh, es))
    return out


def test_oracle_meets_the_contract_and_the_witness_is_not_blind(oracle_mod, witnessed):
    rows = []
    for (dims, name, es), (img, wit) in witnessed.items():
        (w, h), (ow, oh) = dims
        tag = f"{w}x{h}->{ow}x{oh} {name} easu {es}"
        e = oracle_mod.fsr_easu(img, ow, oh, es)
        st = F.fsr_contract(e, wit, "oracle " + tag)
        share = st["single"] / st["samples"]
        rows.append((tag, st["samples"], share, st["differ_from_floor"] / st["samples"]))
        if name in ("noise", "gradient") and (w, h) != (1, 1) and not (name == "gradient" and dims == ((20, 20), (20, 20))):
            floor = 0.85 if dims == ((64, 36), (96, 54)) else 0.95
            assert share >= floor, (tag, share)
        for rs in F.RCAS_SHARPNESS:
            st = F.fsr_contract(oracle_mod.fsr_rcas(e, rs), F.rcas64(e, rs), f"oracle {tag} -> rcas {rs}")
            assert st["decided"] == st["samples"]
            if rs == 0.0:
                assert st["single"] == st["samples"]  # unpack -> pack: the table decides every sample
            rows.append((f"{tag} -> rcas {rs}", st["samples"], st["single"] / st["samples"], st["differ_from_floor"] / st["samples"]))
    w, h = F.RCAS_CASE
    for name, img in F.contents(oracle_mod, w, h).items():
        for rs in F.RCAS_SHARPNESS:
            F.fsr_contract(oracle_mod.fsr_rcas(img, rs), F.rcas64(img, rs), f"oracle {w}x{h} {name} rcas {rs}")
    print("\ncase: samples, single-valued share, share differing from floor(v)")
    for tag, n, share, differ in rows:
        print(f"  {tag}: {n}, {share:.4f}, {differ:.4f}")


def test_the_contract_has_teeth(oracle_mod, witnessed):
    """One-edit mutants of the f32 twin over the same inputs: each puts more than 1 000 samples outside the permitted set."""
    counts = dict.fromkeys(MUTANTS, 0)
    for (dims, name, es), (img, wit) in witnessed.items():
        (w, h), (ow, oh) = dims
        if name == "noise":  # the local copy is the oracle, bit for bit, before it is edited
            assert np.array_equal(_twin(img, ow, oh, es), oracle_mod.fsr_easu(img, ow, oh, es))
        for m in MUTANTS:
            counts[m] += F.fsr_contract(_twin(img, ow, oh, es, m), wit, m, raise_on_violation=False)["violations"]
    print("\nsamples outside the permitted set, per mutant:", counts)
    assert min(counts.values()) > 1000, counts


def _fma(a, b, c):
    """One rounding: the product of two f32 is exact in float64, the sum there errs by 2^-53."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(_f)


def _fast_model(img, ow, oh, sharp):
    """A numpy f32 model of the FAST arithmetic as DESIGN.md states it: the shader's distances and direction weight, FsrCubic from
    a table of 128 cells per unit (value at the left end, difference to the right end, each cell inside one piece; d = 2 keeps its
    weight, anything beyond gets none), FMA sums, reciprocal + one Newton step."""
    ih, iw = img.shape[:2]

    def piece(d, near):
        d2 = d * d
        d3 = d * d2
        return _f(2.0) - _f(1.5) * d - _f(0.5) * d3 + d2 if near else _f(0.0) - _f(0.5) * d + _f(2.5) * d2 - d3

    i = np.arange(257)
    a, b, near = (i / 128.0).astype(_f), ((i + 1) / 128.0).astype(_f), i < 128
    va = np.where(near, piece(a, True), piece(a, False)).astype(_f)
    slope = (np.where(near, piece(b, True), piece(b, False)).astype(_f) - va).astype(_f)
    slope[256] = _f(-1.0e9)
    gx, gy = np.meshgrid(np.arange(ow), np.arange(oh))
    cx, cy = (gx.astype(_f) + _f(0.5)) * (_f(iw) / _f(ow)), (gy.astype(_f) + _f(0.5)) * (_f(ih) / _f(oh))
    ix, iy = cx.astype(np.int32), cy.astype(np.int32)
    fx, fy = cx - np.floor(cx), cy - np.floor(cy)

    def fetch(x, y):
        return img[np.clip(y, 0, ih - 1), np.clip(x, 0, iw - 1), :3].astype(_f) / _f(255.0)

    p, q = np.abs(fetch(ix, iy - 1) - fetch(ix, iy + 1)), np.abs(fetch(ix - 1, iy) - fetch(ix + 1, iy))
    dx, dy = (p[..., 0] + p[..., 1] + p[..., 2]) / _f(3.0) + _f(0.0001), (q[..., 0] + q[..., 1] + q[..., 2]) / _f(3.0) + _f(0.0001)
    ln = np.sqrt(dx * dx + dy * dy)
    dx, dy = dx / ln, dy / ln
    wx = dx / (dx + dy)
    wy = _f(1.0) - wx
    acc, accw = np.zeros((oh, ow, 3), _f), np.zeros((oh, ow), _f)
    for y in range(4):
        for x in range(4):
            ds = np.abs((_f(x) - fx) * wx + (_f(y) - fy) * wy) * _f(128.0)  # scaling by 128 is exact
            cell = np.minimum(ds.astype(np.int64), 256)
            wgt = np.maximum(_fma(np.where(ds >= 257, _f(1.0), ds - np.floor(ds)), slope[cell], va[cell]), _f(0.0))
            acc = _fma(fetch(ix - 1 + x, iy - 1 + y), wgt[..., None], acc)
            accw = accw + wgt
    z = _f(1.0) / accw
    z = z * _fma(-accw, z, _f(2.0))
    col = acc * z[..., None]
    s = _f(sharp)
    if s > _f(0.001):
        col = _fma(col, _f(1.0) - s, fetch(ix, iy) * s)
    out = np.full((oh, ow, 4), 255, np.uint8)
    out[..., :3] = (np.minimum(np.maximum(col, _f(0.0)), _f(1.0)) * _f(255.0)).astype(np.uint32)
    return out


def test_fast_arithmetic_meets_the_fast_contract(oracle_mod):
    """eps_fast is derived from the definition of the table; a plain model of that arithmetic must fit inside it, differ from the
    oracle somewhere, and keep the shares."""
    differs = 0
    for dims in F.CASES:
        (w, h), (ow, oh) = dims
        for name, img in F.contents(oracle_mod, w, h).items():
            for es in F.EASU_SHARPNESS:
                got = _fast_model(img, ow, oh, es)
                st = F.fsr_contract(got, F.easu64(img, ow, oh, es, fast=True), f"FAST model {w}x{h}->{ow}x{oh} {name} {es}")
                differs += int((got != oracle_mod.fsr_easu(img, ow, oh, es)).sum())
                if name in ("noise", "gradient") and (w, h) != (1, 1) and not (name == "gradient" and dims == ((20, 20), (20, 20))):
                    assert st["single"] / st["samples"] >= (0.85 if dims == ((64, 36), (96, 54)) else 0.95), (dims, name, es)
    assert differs > 0


def test_rcas_contract_has_teeth(oracle_mod):
    """RCAS: every byte one count up, the luma weights applied in the wrong channel order, another sharpness -- each more than
    1 000 of 20 736 samples outside."""
    img = oracle_mod.fsr_easu(oracle_mod.gen_noise(24, 18, 9), 96, 72, 0.0)  # smooth: low contrast, the sharpening is at work
    wit = F.rcas64(img, 0.7)
    good = oracle_mod.fsr_rcas(img, 0.7)
    assert F.fsr_contract(good, wit, "oracle")["violations"] == 0
    one_up = good.copy()
    one_up[..., :3] = np.minimum(good[..., :3].astype(np.int16) + 1, 255)
    bgr = oracle_mod.fsr_rcas(img[..., [2, 1, 0, 3]].copy(), 0.7)[..., [2, 1, 0, 3]]  # luma weights applied in the wrong order
    for tag, bad in (("one count up", one_up), ("luma of BGR", bgr), ("sharpness 0.6", oracle_mod.fsr_rcas(img, 0.6))):
        n = F.fsr_contract(bad, wit, tag, raise_on_violation=False)["violations"]
        print(tag, n)
        assert n > 1000, (tag, n)


def test_witness_alone(oracle_mod):
    flat = np.full((9, 11, 4), 77, np.uint8)
    for (ow, oh), es in (((22, 18), 0.0), ((25, 13), 0.3), ((11, 9), 0.0), ((7, 5), 0.3)):
        for fast in (False, True):
            wit = F.easu64(flat, ow, oh, es, fast=fast)
            assert np.abs(wit.v - 77.0).max() < 1e-9
            lo, hi = F.permitted(wit)
            assert (lo == 76).all() and (hi == 77).all()  # on the integer: both neighbours, never one
    r = F.rcas64(flat, 0.9)
    assert np.abs(r.v - 77.0).max() < 1e-9 and (r.pinned == -1).all()
    # EASU commutes with transposition (FsrDirA's two gradients and the two offsets swap together); it does NOT commute with a
    # mirror: the taps span ix - 1 .. ix + 2 around a sample at ix + fx and the distance adds px wx and py wy WITH their signs
    # (fsr.rs:117, :142-145).  RCAS's five taps are symmetric, so it does.
    img = oracle_mod.gen_noise(20, 12, 3)
    for (ow, oh), es in (((40, 24), 0.3), ((31, 17), 0.0), ((20, 12), 0.3)):
        a, t = F.easu64(img, ow, oh, es), F.easu64(img.transpose(1, 0, 2).copy(), oh, ow, es)
        assert np.abs(a.v - t.v.transpose(1, 0, 2)).max() < 1e-9
        assert np.array_equal(a.decided, t.decided.transpose(1, 0, 2))
    a, m = F.rcas64(img, 0.7), F.rcas64(img[:, ::-1].copy(), 0.7)
    assert np.abs(a.v - m.v[:, ::-1]).max() < 1e-9 and np.array_equal(a.pinned, m.pinned[:, ::-1])
    # RCAS at sharpness 0 returns v on the integers, and the byte is the table's: C or C - 1
    z = F.rcas64(img, 0.0)
    c = img[..., :3].astype(np.int16)
    assert np.abs(z.v - c).max() < 1e-9 and np.array_equal(z.pinned, F.PACK_OF_UNPACK[img[..., :3]])
    assert ((F.PACK_OF_UNPACK == np.arange(256)) | (F.PACK_OF_UNPACK == np.arange(256) - 1)).all()
    assert np.array_equal(oracle_mod.fsr_rcas(img, 0.0)[..., :3], z.pinned)
    # x3/2: every third column and row has fract = 0; where both do, tap (2, 2) sits at d = 2 wx + 2 wy = 2: undecided
    g = F.easu64(oracle_mod.gen_noise(8, 8, 1), 12, 12, 0.0)
    assert not g.decided[1::3, 1::3].any() and g.decided[0::3].all() and g.decided[:, 2::3].all()
