"""The lane exchange of k_lanczos3_x2's horizontal pass (nus_k_lanczos_x2.hip, lanczos_x2_hpass), checked on the code hipcc
generates (no GPU needed).  The five FMA-mode six-tap instantiations fetch their six halo values per channel from LDS and must
stay at three waves per SIMD doing so -- two earlier LDS exchanges lost on exactly that: registers, spills, a block's LDS -- ; the
EXACT and NARROW instantiations keep the DPP moves."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(exact, blend, unit, narrow): (metadata block, body)} of the twelve instantiations, compiled as tests/test_kernel_asm.py does."""
    import check_hidden_loads as chk

    out = tmp_path_factory.mktemp("asm") / "nus_k_lanczos_x2.s"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
           "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out),
           os.path.join(CSRC, "nus_k_lanczos_x2.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    text = out.read_text()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        meta[re.search(r"\.name:\s*(\S+)", m.group(0)).group(1)] = m.group(0)
    found = {}
    for name, body in chk.kernel_bodies(text, "k_lanczos3_x2IL"):
        e, b, u, n = re.search(r"k_lanczos3_x2ILb([01])ELi(\d)ELb([01])ELb([01])E", name).groups()
        found[(e == "1", int(b), u == "1", n == "1")] = (meta[name], body)
    assert len(found) == 12, sorted(found)
    return found


def _field(meta, key):
    return int(re.search(r"\.%s:\s*(\d+)" % key, meta).group(1))


FMA_SIX_TAP = [(False, 0, False, False), (False, 1, False, False), (False, 2, False, False), (False, 1, True, False),
               (False, 2, True, False)]  # plain, blend 1/2, blend t, unit 1/2, unit t


@pytest.mark.parametrize("key", FMA_SIX_TAP, ids=["plain", "blend_half", "blend_t", "unit_half", "unit_t"])
def test_fma_six_tap_kernels_exchange_through_lds_at_three_waves_per_simd(kernels, key):
    meta, body = kernels[key]
    assert _field(meta, "vgpr_count") <= 168, _field(meta, "vgpr_count")  # 512 / 3, in allocation granules of 8
    assert _field(meta, "vgpr_spill_count") == 0
    assert _field(meta, "private_segment_fixed_size") == 0  # no scratch: a reload would be a vmcnt-counted load in the loop
    assert 3 * _field(meta, "group_segment_fixed_size") <= 160 * 1024
    assert "_dpp" not in body
    assert "ds_read2_b32" in body


def test_exact_and_narrow_kernels_still_exchange_by_dpp(kernels):
    others = [k for k in kernels if k not in FMA_SIX_TAP]
    assert len(others) == 7 and all(k[0] or k[3] for k in others)  # EXACT x (BLEND 0 - 2, UNIT 1 - 2), NARROW x EXACT
    for key in others:
        meta, body = kernels[key]
        assert re.search(r"v_mov_b32_dpp .* wave_sh[lr]:1", body), key
        assert "ds_read2_b32" not in body, key
        assert _field(meta, "vgpr_spill_count") == 0 and _field(meta, "private_segment_fixed_size") == 0, key
