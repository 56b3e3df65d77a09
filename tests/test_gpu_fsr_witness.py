"""GPU: the FSR1 HIP kernels, EXACT and FAST, held directly to the float64 witness of the two shaders (tests/_fsr64.py) -- not
through the C oracle, which the same witness holds on the CPU (tests/test_fsr64_contract.py).  No reference-held vector exists
for either pass (the reference never dispatches the shaders, fsr.rs:24-260); this witness is what pins them.

Every case runs three frames (noise, gradient, edge) through the device path, outputs between guard bands, and asserts its
kernel_variant: as ONE batch, so that frame strides count, wherever upscale_device takes one (frame sizes that are multiples of 16
bytes), one by one at the odd sizes.  `easu` against easu64 of the input, `fsr1` against rcas64 of the EASU image the SAME mode produced
(RCAS amplifies a count of its centre tap, so the pair is held pass by pass), `rcas` alone at one strip plus a column and one
row block plus a row of the row walker.  The sizes are the smallest that reach each path of launch_fsr1:

  (32,24)->(64,48)      x2, 16-byte stores, the FAST quad form; also run with BGRA, RGBX and BGRX input against the witness of
                        the converted frame
  (17,13)->(40,29)      ragged tiles
  (100,70)->(257,131)   width not a multiple of 4, several 64 x 32 tiles
  (5,3)->(130,67)       clamped taps everywhere
  (64,36)->(96,54)      x3/2 (one sample in nine undecided)
  (70,40)->(64,33)      footprint over the LDS cap: taps from memory, FAST falls back to the exact arithmetic (equal to the oracle)
  (20,20)->(20,20)      x1
  (1,1)->(3,2)          the smallest frame

FAST's contract is the witness with the table's interpolation error added per sample, eps_fast in tests/_fsr64.py:
2 / (8 128^2) = 1.53e-5 per weight on d <= 1, 7 / (8 128^2) = 5.34e-5 on 1 < d <= 2, 2 U for the stored entries and K = 38 for 35
(reciprocal + Newton step).  Measured on a numpy f32 model of that arithmetic, single-valued share of the samples (EXACT in
brackets): noise 0.994-0.998 (0.998-0.999), gradient 0.997-1.0 (0.998-1.0), x3/2 0.884-0.889 (0.887-0.889), the gradient at x1
0.590 (0.590); the last test prints the table measured on the device.  Whether FAST ran is decided by its bytes differing from
the oracle's somewhere, at the sizes of 64 x 36 and more where it can.

The two-pass threshold (frames of 1 MiB and more take EASU into scratch images, then the row-walking RCAS) is crossed at its
smallest size: (256,256)->(512,512) is exactly 1 MiB, five frames so that the four-frame scratch chunks wrap; (512,511) stays
fused; fsr_two_pass = 0 gives the same bytes."""
import numpy as np
import pytest

import _fsr64 as F
from conftest import guarded  # device outputs between poisoned guard bands (tests/conftest.py)
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch  # host <-> HBM through nus_upload / nus_download

pytestmark = pytest.mark.gpu

VARIANTS = {"fsr1_easu_tile", "fsr1_easu_rcas_fused_lds", "fsr1_rcas_rows", "fsr1_easu_then_rcas_rows"}
_STATS = {}  # (kernel_variant, mode) -> [samples, single-valued, differing from floor(v)]
_WITNESS = {}  # computed once per (image, size, sharpness, mode), left unchanged


def _record(variant, fast, st):
    s = _STATS.setdefault((variant, "FAST" if fast else "EXACT"), [0, 0, 0])
    s[0] += st["samples"]
    s[1] += st["single"]
    s[2] += st["differ_from_floor"]


def _frames(oracle_mod, w, h):
    c = F.contents(oracle_mod, w, h)
    return np.stack([c["noise"], c["gradient"], c["edge"]])


def _easu64(key, img, ow, oh, es, fast):
    k = (key, ow, oh, es, fast)
    if k not in _WITNESS:
        _WITNESS[k] = F.easu64(img, ow, oh, es, fast=fast)
    return _WITNESS[k]


def _device(nsc, alg, frames, ow, oh, fast=False, easu=-1.0, rcas=-1.0, fmt="rgba", options=()):
    import torch
    u = nsc.PyWgpuUpscaler("quality", alg)
    if fast:
        u.set_option("fsr_fast", 1)
    for k, v in options:
        u.set_option(k, v)
    u.set_input_format(fmt)
    u.set_sharpness(easu, rcas)
    n, h, w = frames.shape[:3]
    u.initialize(w, h, ow, oh)
    stream = torch.cuda.current_stream().cuda_stream
    if (w * h * 4) % 16 == 0 and (ow * oh * 4) % 16 == 0:
        d_in = put(np.ascontiguousarray(frames))
        d_out = guarded.empty((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
        u.upscale_device(d_in.data_ptr(), d_out.data_ptr(), n, stream)
        torch.cuda.synchronize()
        return fetch(d_out), u.kernel_variant
    outs = []  # upscale_device takes a batch only of frames whose sizes are multiples of 16 bytes: these go one by one
    for k in range(n):
        d_in = put(np.ascontiguousarray(frames[k]))
        d_out = guarded.empty((oh, ow, 4), dtype=torch.uint8, device="cuda")
        u.upscale_device(d_in.data_ptr(), d_out.data_ptr(), 1, stream)
        torch.cuda.synchronize()
        outs.append(fetch(d_out))
    return np.stack(outs), u.kernel_variant


def _hold_pair(nsc, frames, key, ow, oh, es, fast, fmt="rgba", converted=None):
    """easu and fsr1 of one batch in one mode: EASU against the witness of the (converted) input, the pair's RCAS against the
    witness of the EASU image this mode produced.  Returns the EASU images."""
    mode = "FAST" if fast else "EXACT"
    src = frames if converted is None else converted
    n, h, w = frames.shape[:3]
    got_e, variant = _device(nsc, "easu", frames, ow, oh, fast=fast, easu=es, fmt=fmt)
    assert variant == "fsr1_easu_tile"
    for k in range(n):
        st = F.fsr_contract(got_e[k], _easu64((key, k), src[k], ow, oh, es, fast), f"{mode} easu {w}x{h}->{ow}x{oh} {fmt} frame {k} sharpness {es}")
        _record(variant, fast, st)
    got_f, variant = _device(nsc, "fsr1", frames, ow, oh, fast=fast, easu=es, rcas=0.7, fmt=fmt)
    assert variant == "fsr1_easu_rcas_fused_lds"
    for k in range(n):
        st = F.fsr_contract(got_f[k], F.rcas64(got_e[k], 0.7), f"{mode} fsr1 {w}x{h}->{ow}x{oh} {fmt} frame {k} sharpness {es}")
        _record(variant, fast, st)
    return got_e


@pytest.mark.parametrize("dims", F.CASES)
def test_easu_and_fused_pair_meet_the_witness(nsc, oracle_mod, dims):
    (w, h), (ow, oh) = dims
    frames = _frames(oracle_mod, w, h)
    differs = False
    for es in F.EASU_SHARPNESS:
        exact = _hold_pair(nsc, frames, dims, ow, oh, es, fast=False)
        fast = _hold_pair(nsc, frames, dims, ow, oh, es, fast=True)
        want = np.stack([oracle_mod.fsr_easu(f, ow, oh, es) for f in frames])
        assert np.array_equal(exact, want)  # EXACT stays bit-exact (tests/test_fsr1.py holds that at more sizes)
        differs = differs or not np.array_equal(fast, want)
    if dims == ((70, 40), (64, 33)):
        assert not differs, "FAST over the LDS cap runs the exact arithmetic"
    elif w * h >= 64 * 36:
        assert differs, "the FAST kernel did not run"


@pytest.mark.parametrize("fmt", ["bgra", "rgbx", "bgrx"])
def test_input_formats_meet_the_witness_on_the_converted_frames(nsc, oracle_mod, fmt):
    (w, h), (ow, oh) = F.CASES[0]
    rgba = _frames(oracle_mod, w, h)
    rgba[..., 3] = oracle_mod.gen_noise(w, h, 5)[..., 0]  # an alpha (or X) byte that must not matter: both passes write 255
    frames = np.ascontiguousarray(rgba[..., [2, 1, 0, 3]]) if fmt[0] == "b" else rgba
    for fast in (False, True):
        _hold_pair(nsc, frames, F.CASES[0], ow, oh, 0.3, fast=fast, fmt=fmt, converted=rgba)


def test_rcas_alone_meets_the_witness(nsc, oracle_mod):
    w, h = F.RCAS_CASE
    frames = _frames(oracle_mod, w, h)
    for rs in F.RCAS_SHARPNESS:
        got, variant = _device(nsc, "rcas", frames, w, h, rcas=rs)
        assert variant == "fsr1_rcas_rows"
        for k in range(len(frames)):
            _record(variant, False, F.fsr_contract(got[k], F.rcas64(frames[k], rs), f"rcas {w}x{h} frame {k} sharpness {rs}"))
            assert np.array_equal(got[k], oracle_mod.fsr_rcas(frames[k], rs))
    got, variant = _device(nsc, "rcas", frames, w, h, fast=True, rcas=0.7)  # fsr_fast leaves RCAS alone
    assert variant == "fsr1_rcas_rows"
    for k in range(len(frames)):
        _record(variant, True, F.fsr_contract(got[k], F.rcas64(frames[k], 0.7), f"FAST rcas {w}x{h} frame {k}"))


def test_two_pass_threshold_both_sides(nsc, oracle_mod):
    w = h = 256
    frames = np.stack([oracle_mod.gen_noise(w, h, 40), oracle_mod.gen_gradient(w, h), F.contents(oracle_mod, w, h)["edge"],
                       oracle_mod.gen_gradient(w, h, 2), oracle_mod.gen_noise(w, h, 41)])
    want = np.stack([oracle_mod.fsr1(f, 512, 512, 0.0, 0.7) for f in frames])
    got, variant = _device(nsc, "fsr1", frames, 512, 512, easu=0.0, rcas=0.7)  # exactly 1 MiB per frame: two passes, 4 + 1 frames
    assert variant == "fsr1_easu_then_rcas_rows"
    assert np.array_equal(got, want)
    fused, variant = _device(nsc, "fsr1", frames, 512, 512, easu=0.0, rcas=0.7, options=(("fsr_two_pass", 0),))
    assert variant == "fsr1_easu_rcas_fused_lds"
    assert np.array_equal(fused, got)
    below, variant = _device(nsc, "fsr1", frames, 512, 511, easu=0.0, rcas=0.7)  # 4 * 512 * 511 < 1 MiB
    assert variant == "fsr1_easu_rcas_fused_lds"
    assert np.array_equal(below, np.stack([oracle_mod.fsr1(f, 512, 511, 0.0, 0.7) for f in frames]))
    # the witness on the two-pass path, both modes; the last frame is the one the second scratch chunk holds
    k = len(frames) - 1
    e_exact = oracle_mod.fsr_easu(frames[k], 512, 512, 0.0)
    _record("fsr1_easu_then_rcas_rows", False, F.fsr_contract(got[k], F.rcas64(e_exact, 0.7), "EXACT two-pass"))
    e_fast, variant = _device(nsc, "easu", frames, 512, 512, fast=True, easu=0.0)
    assert variant == "fsr1_easu_tile"
    _record(variant, True, F.fsr_contract(e_fast[k], F.easu64(frames[k], 512, 512, 0.0, fast=True), "FAST easu 256->512"))
    assert not np.array_equal(e_fast[k], e_exact), "the FAST kernel did not run"
    f_fast, variant = _device(nsc, "fsr1", frames, 512, 512, fast=True, easu=0.0, rcas=0.7)
    assert variant == "fsr1_easu_then_rcas_rows"
    for j in range(len(frames)):
        assert np.array_equal(f_fast[j], oracle_mod.fsr_rcas(e_fast[j], 0.7)), j
    _record(variant, True, F.fsr_contract(f_fast[k], F.rcas64(e_fast[k], 0.7), "FAST two-pass"))


def test_every_fsr_variant_was_held_in_both_modes():
    """Runs last: the table of what the tests above held."""
    print("\n(kernel_variant, mode): samples, single-valued share, share differing from floor(v)")
    for key in sorted(_STATS):
        n, single, differ = _STATS[key]
        print(f"  {key}: {n}, {single / n:.4f}, {differ / n:.5f}")
    assert {v for v, _ in _STATS} == VARIANTS
    assert {(v, m) for v in VARIANTS for m in ("EXACT", "FAST")} == set(_STATS)
