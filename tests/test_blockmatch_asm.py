"""The block-matching kernels (nus_k_blockmatch.hip) as hipcc builds them for gfx950, checked without a GPU: no scratch and no
spills, no atomics, an LDS budget that lets two search workgroups share a CU, and the byte-SAD instruction on the search's path."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")
KERNELS = ("k_bm_search", "k_bm_rough", "k_bm_refine", "k_bm_zero_flags", "k_bm_flow")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def bm_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("asm") / "nus_k_blockmatch.s"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
           "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out),
           os.path.join(CSRC, "nus_k_blockmatch.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return out.read_text()


def _bodies(asm):
    """{mangled kernel name: its instruction text} for every block-matching kernel."""
    out = {}
    for m in re.finditer(r"^(_Z\S*(?:%s)\S*):" % "|".join(KERNELS), asm, re.M):
        end = asm.find(".Lfunc_end", m.end())
        out[m.group(1)] = asm[m.end():end]
    return out


def test_built_with_the_makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-O3 -std=c++17 -fPIC -ffp-contract=off" in mk
    assert "nus_k_blockmatch.hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0]


def test_every_instantiation_is_there(bm_asm):
    names = list(_bodies(bm_asm))
    for k in KERNELS:
        assert any(k in n for n in names), (k, names)
    assert sum("k_bm_search" in n for n in names) == 3  # block sizes 8, 16, 32
    assert sum("k_bm_flow" in n for n in names) == 2    # f32 and f16
    assert all("s_endpgm" in body for body in _bodies(bm_asm).values())


def test_no_scratch_no_spills(bm_asm):
    found = 0
    for m in re.finditer(r"^\s+\.name:\s+(\S+)\s*$", bm_asm, re.M):
        name = m.group(1)
        if not any(k in name for k in KERNELS) or name.endswith(".kd"):
            continue
        block = bm_asm[m.start():m.start() + 4000]
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        assert priv and int(priv.group(1)) == 0, (name, priv and priv.group(0))
        for key in ("sgpr_spill_count", "vgpr_spill_count"):
            sp = re.search(r"\.%s:\s+(\d+)" % key, block)
            assert sp and int(sp.group(1)) == 0, (name, key, sp and sp.group(0))
        found += 1
    assert found >= 8
    for name, body in _bodies(bm_asm).items():
        assert "scratch_" not in body and "buffer_store" not in body, name


def test_no_atomics(bm_asm):
    for name, body in _bodies(bm_asm).items():
        assert "atomic" not in body and "cmpswap" not in body, name
        assert not re.search(r"\bds_(add|min|max|and|or|xor|cmpst)", body), name


def test_byte_sad_instruction_on_the_search_path(bm_asm):
    for name, body in _bodies(bm_asm).items():
        if "k_bm_search" in name:
            bs = int(re.search(r"k_bm_searchILi(\d+)E", name).group(1))
            # 2 candidates x bs pixels per block row, in the full-width and in the partial-width form of the row loop
            assert body.count("v_sad_u8") == 4 * bs, (name, body.count("v_sad_u8"))


def test_lds_lets_two_workgroups_share_a_cu(nsc):
    """The search's LDS is dynamic: (2R + bs) rows of 2R + 66 dwords (bm_lds_bytes), plus the few static words of the reduction."""
    worst = 0
    for bs in (8, 16, 32):
        for R in range(1, nsc._capi.BM_MAX_RADIUS + 1):
            worst = max(worst, (2 * R + bs) * (2 * R + 2 + 64) * 4 + 64)
    assert worst == (48 + 32) * 114 * 4 + 64
    assert 2 * worst <= LDS_PER_CU
    src = open(os.path.join(CSRC, "nus_k_blockmatch.hip")).read()
    assert "return (size_t)(2 * R + bs) * (2 * R + 2 + kBmRunPixels) * 4;" in src
    assert "constexpr uint32_t kBmRunPixels = 64;" in open(os.path.join(CSRC, "nus_kernels.hpp")).read()


def test_static_lds_is_small(bm_asm):
    sizes = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", bm_asm)]
    assert len(sizes) == 8 and max(sizes) <= 64, sizes
