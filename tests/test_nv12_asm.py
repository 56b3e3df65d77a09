"""The two NV12 kernel units (nus_k_nv12.hip, nus_k_nv12_resize.hip) as hipcc builds them for gfx950, checked without a GPU, in
the manner of tests/test_yuv_asm.py: every template instance is there and nothing else, none uses scratch or spills, none has
static LDS (the conversions and the repack use no LDS and the pair row kernel's is dynamic), every k_pair_rows instance stays
within the 128 VGPRs that leave four waves per SIMD and uses no AGPRs, and the conversion unit holds no v_ashr_pk_u8_i32 (the fused
shift that yuv_pixel's comment in nus_yuv_device.hpp describes: it gave wrong third bytes on the MI355X)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")
# kernel name with its template arguments as the Itanium mangling spells them (Li<n>E an int, Lb<n>E a bool)
NV12 = tuple(f"k_nv12_to_rgbaILi{f}ELi{s}EE" for f in (0, 1) for s in (0, 1)) + \
       tuple(f"k_nv12_to_rgba_pxILi{f}ELi{s}EE" for f in (0, 1) for s in (0, 1)) + \
       tuple(f"k_rgba_to_nv12ILi{s}EE" for s in (0, 1)) + tuple(f"k_rgba_to_nv12_cellILi{s}EE" for s in (0, 1)) + \
       tuple(f"k_nv12_repackILb{d}ELb{v}EE" for d in (0, 1) for v in (0, 1))
RESIZE = tuple(f"k_pair_rowsILb{e}ELi8EE" for e in (0, 1)) + tuple(f"k_pair_pxILb{e}EE" for e in (0, 1))
UNITS = {"nus_k_nv12": NV12, "nus_k_nv12_resize": RESIZE}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """{unit: its assembly text}."""
    out = {}
    for unit in UNITS:
        path = tmp_path_factory.mktemp("asm") / (unit + ".s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
               "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(path),
               os.path.join(CSRC, unit + ".hip")]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        out[unit] = path.read_text()
    return out


def _metadata(text):
    """{mangled kernel name: {key: int}} from the amdhsa.kernels list of the unit's metadata."""
    kernels = {}
    for entry in re.split(r"^  - (?=\.)", text[text.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)\s*$", entry, re.M).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return kernels


def _find(meta, instance):
    """The one kernel whose mangled name holds `<length>k_...<template arguments>`, the end of the nested name and a void return."""
    hits = [n for n in meta if re.search(r"\d+" + re.escape(instance) + "Ev", n)]
    assert len(hits) == 1, (instance, sorted(meta))
    return hits[0]


def test_built_with_the_makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-O3 -std=c++17 -fPIC -ffp-contract=off" in mk
    for unit in UNITS:
        assert unit + ".hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0]


def test_every_kernel_is_there(asm):
    assert (len(NV12), len(RESIZE)) == (16, 4)
    for unit, instances in UNITS.items():
        meta = _metadata(asm[unit])
        assert len(meta) == len(instances), (unit, sorted(meta))
        assert len({_find(meta, i) for i in instances}) == len(instances), unit
        for name in meta:  # the code is there as well, not the descriptor alone
            body = asm[unit][asm[unit].index("\n" + name + ":"):]
            assert "s_endpgm" in body[:body.index(".Lfunc_end")], name


def test_no_scratch_no_spills_and_no_static_lds(asm):
    seen = 0
    for unit in UNITS:
        for name, m in _metadata(asm[unit]).items():
            assert m["private_segment_fixed_size"] == 0, (name, "scratch: the head comment of " + unit + ".hip says none")
            assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name
            assert m["group_segment_fixed_size"] == 0, (name, "static LDS")
            seen += 1
    assert seen == 20


def test_the_pair_row_kernel_leaves_four_waves_per_simd(asm):
    """512 VGPRs per SIMD lane: four waves need at most 128 each."""
    meta = _metadata(asm["nus_k_nv12_resize"])
    rows = [i for i in RESIZE if i.startswith("k_pair_rows")]
    assert len(rows) == 2
    for inst in rows:
        m = meta[_find(meta, inst)]
        print(inst, m["vgpr_count"], "VGPRs", m["agpr_count"], "AGPRs")
        assert m["vgpr_count"] <= 128 and m["agpr_count"] == 0, (inst, m["vgpr_count"], m["agpr_count"])


def test_the_conversions_hold_no_fused_shift(asm):
    n = asm["nus_k_nv12"].count("v_ashr_pk_u8_i32")
    assert n == 0, (f"{n} v_ashr_pk_u8_i32 in nus_k_nv12.s: the compiler has fused yuv_pixel's shifts with its clamps, which gave wrong "
                    "third bytes on the MI355X -- see the comment in yuv_pixel (nus_yuv_device.hpp) and keep the shifts apart")
