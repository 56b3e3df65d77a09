"""The warp + blend kernels (nus_k_interp.hip) as hipcc builds them for gfx950, checked without a GPU: no instantiation spills to
scratch, and the multi-time forms read their inputs once -- the vector zero-flow kernel's body holds exactly two 16-byte global
loads (A and B) whatever the number of times, and a multi-time dense kernel loads the flow as its single-time form does."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")


@pytest.fixture(scope="module")
def interp_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("asm") / "nus_k_interp.s"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
           "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out),
           os.path.join(CSRC, "nus_k_interp.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return out.read_text()


def _bodies(asm):
    """{mangled kernel name: its instruction text} for every warp / blend kernel."""
    out = {}
    for m in re.finditer(r"^(_Z\S*(?:k_blend_zero_flow|k_warp_blend_flow)\S*):", asm, re.M):
        end = asm.find(".Lfunc_end", m.end())
        out[m.group(1)] = asm[m.end():end]
    return out


def _count(body, pattern):
    return len(re.findall(r"^\s+" + pattern + r"\b", body, re.M))


def test_built_with_the_makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-O3 -std=c++17 -fPIC -ffp-contract=off" in mk
    assert "nus_k_interp.hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0]


def test_every_instantiation_is_there(interp_asm):
    names = list(_bodies(interp_asm))
    zero = [n for n in names if "k_blend_zero_flow" in n]
    dense = [n for n in names if "k_warp_blend_flowI" in n]
    assert len(zero) == 4, zero      # VEC x MT
    assert len(dense) == 16, dense   # MODE x HALF x (XV = 2, 1) x MT
    assert sum("k_warp_blend_flow_tiny" in n for n in names) == 2  # MT
    assert sum(n.split("EEEv")[0].endswith("ELb1") for n in dense) == 8  # the multi-time forms (last template argument)


def test_no_scratch(interp_asm):
    found = 0
    for m in re.finditer(r"^\s+\.name:\s+(\S+)\s*$", interp_asm, re.M):
        name = m.group(1)
        if not re.search(r"k_blend_zero_flow|k_warp_blend_flow", name) or name.endswith(".kd"):
            continue
        block = interp_asm[m.start():m.start() + 4000]
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        assert priv and int(priv.group(1)) == 0, (name, priv and priv.group(0))
        found += 1
    assert found == 22
    for name, body in _bodies(interp_asm).items():
        assert "scratch_" not in body, name


def test_vector_zero_flow_kernel_reads_a_and_b_once(interp_asm):
    vec = {n: b for n, b in _bodies(interp_asm).items() if "k_blend_zero_flowILb1E" in n}
    assert len(vec) == 2
    for name, body in vec.items():
        loads = re.findall(r"^\s+((?:global|buffer|flat)_load\w*)", body, re.M)
        assert loads == ["global_load_dwordx4", "global_load_dwordx4"], (name, loads)
    multi = next(b for n, b in vec.items() if "k_blend_zero_flowILb1ELb1E" in n)
    assert _count(multi, "global_store_dwordx4") == 1      # one 16-byte store per time, in the loop over the set
    assert re.search(r"^\s+s_cbranch_\w+\s+\.LBB", multi, re.M)


def test_multi_time_dense_kernels_load_the_flow_once(interp_asm):
    bodies = _bodies(interp_asm)
    checked = 0
    for name, body in bodies.items():
        if "k_warp_blend_flowI" not in name or not name.split("EEEv")[0].endswith("ELb1"):
            continue
        single = bodies[name.replace("ELb1EEEv", "ELb0EEEv", 1)]
        assert _count(body, r"global_load\w*") == _count(single, r"global_load\w*") > 0, name  # the flow vectors
        assert _count(body, r"global_load\w*") <= 4, name
        checked += 1
    assert checked == 8
