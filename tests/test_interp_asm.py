"""The warp + blend kernels (nus_k_interp.hip) as hipcc builds them for gfx950, checked without a GPU: no instantiation spills to
scratch, and the multi-time forms read their inputs once -- the vector zero-flow kernel's body holds exactly two 16-byte global
loads (A and B) whatever the number of times, and a multi-time dense kernel loads the flow as its single-time form does.  The
same for the two other units built on the dense kernel's tile, nus_k_bm_warp.hip and nus_k_warp_project.hip (at the end)."""
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


# ---- the other two users of warp_blend_tile (nus_warp_device.hpp): the block-vector and the projecting kernels ----

def _compile(tmp_path_factory, unit):
    out = tmp_path_factory.mktemp("asm") / (unit + ".s")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
           "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, unit + ".hip")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return out.read_text()


@pytest.fixture(scope="module")
def bm_warp_asm(tmp_path_factory):
    return _compile(tmp_path_factory, "nus_k_bm_warp")


@pytest.fixture(scope="module")
def warp_project_asm(tmp_path_factory):
    return _compile(tmp_path_factory, "nus_k_warp_project")


def _kernels(asm, pattern):
    """{mangled kernel name: its instruction text} for the kernels whose name matches."""
    out = {}
    for m in re.finditer(r"^(_Z\S*(?:" + pattern + r")\S*):", asm, re.M):
        out[m.group(1)] = asm[m.end():asm.find(".Lfunc_end", m.end())]
    return out


def _private_sizes(asm, pattern):
    """{kernel name: .private_segment_fixed_size} from the code object's metadata."""
    out = {}
    for m in re.finditer(r"^\s+\.name:\s+(\S+)\s*$", asm, re.M):
        if re.search(pattern, m.group(1)) and not m.group(1).endswith(".kd"):
            out[m.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", asm[m.start():m.start() + 4000]).group(1))
    return out


def _is_multi(name):
    return name.split("EEEv")[0].endswith("ELb1")  # MT, the last template argument


def _check_unit(asm, pattern, tile, n_tile, load):
    """The instantiation counts, no scratch, and every multi-time tile kernel issuing its single-time form's vector loads."""
    bodies = _kernels(asm, pattern)
    dense = {n: b for n, b in bodies.items() if tile + "I" in n}
    assert len(dense) == n_tile, sorted(dense)
    assert sum(tile + "_tinyI" in n for n in bodies) == 2  # MT
    assert len(bodies) == n_tile + 2, sorted(bodies)
    assert sum(_is_multi(n) for n in dense) == n_tile // 2
    assert _private_sizes(asm, pattern) == {n: 0 for n in bodies}
    for name, body in bodies.items():
        assert "scratch_" not in body, name
    for name, body in dense.items():
        if _is_multi(name):
            single = dense[name.replace("ELb1EEEv", "ELb0EEEv", 1)]
            assert _count(body, load) == _count(single, load) > 0, name
    return dense


def test_block_vector_warp_kernels(bm_warp_asm):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "nus_k_bm_warp.hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0]
    dense = _check_unit(bm_warp_asm, "k_bm_warp", "k_bm_warp", 8, r"global_load\w*")  # MODE x (XV = 2, 1) x MT
    for name, body in dense.items():
        assert _count(body, r"global_load\w*") == 2, name  # one 4-byte vector per thread row, whatever XV and the number of times


def test_projecting_warp_kernels(warp_project_asm):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "nus_k_warp_project.hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0]
    # MODE x HALF x (XV = 2, 1) x MT.  Every load of these kernels goes through a buffer resource: the thread's own vectors, the
    # rounds' gathers (one rolled loop, so the same instructions for every time) and the frame samples
    dense = _check_unit(warp_project_asm, "k_warp_blend_flow_proj", "k_warp_blend_flow_proj", 16, r"buffer_load\w*")
    for name, body in dense.items():
        assert _count(body, r"(?:global|flat)_load\w*") == 0, name
    assert len(_kernels(warp_project_asm, "k_flow_project")) == 2  # CORNER
