"""The scene-cut kernels (nus_k_scene.hip) as hipcc builds them for gfx950, checked without a GPU: no scratch, no global, flat
or float atomics and no compare-and-swap loop (the determinism rule: per-workgroup partials go to the workspace and a finish kernel adds them), and the
instructions the design rests on are there (v_sad_u8 for the SAD, v_dot4_u32_u8 for the luma, ds_add_u32 for the histogram
columns)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")
KERNELS = ("k_scene_measure", "k_scene_finish", "k_scene_apply")


@pytest.fixture(scope="module")
def scene_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("asm") / "nus_k_scene.s"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
           "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out),
           os.path.join(CSRC, "nus_k_scene.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return out.read_text()


def _bodies(asm):
    """{mangled kernel name: its instruction text} for every scene kernel."""
    out = {}
    for m in re.finditer(r"^(_Z\S*(?:%s)\S*):" % "|".join(KERNELS), asm, re.M):
        name = m.group(1)
        end = asm.find(".Lfunc_end", m.end())
        out[name] = asm[m.end():end]
    return out


def test_built_with_the_makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-O3 -std=c++17 -fPIC -ffp-contract=off" in mk
    assert "nus_k_scene.hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0]


def test_every_kernel_is_there(scene_asm):
    bodies = _bodies(scene_asm)
    for k in KERNELS:
        assert any(k in n for n in bodies), (k, list(bodies))
    assert sum("k_scene_measure" in n for n in bodies) == 1
    assert all("s_endpgm" in body for body in bodies.values())


def test_no_scratch(scene_asm):
    found = 0
    for m in re.finditer(r"^\s+\.name:\s+(\S+)\s*$", scene_asm, re.M):
        name = m.group(1)
        if not any(k in name for k in KERNELS) or name.endswith(".kd"):
            continue
        block = scene_asm[m.start():m.start() + 4000]
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        assert priv and int(priv.group(1)) == 0, (name, priv and priv.group(0))
        found += 1
    assert found >= 3
    for name, body in _bodies(scene_asm).items():
        assert "scratch_" not in body and "buffer_store" not in body, name


def test_no_global_or_float_atomics_or_cmpswap(scene_asm):
    for name, body in _bodies(scene_asm).items():
        for bad in ("global_atomic", "flat_atomic", "buffer_atomic", "atomic_add_f", "atomic_pk_add", "cmpswap", "ds_add_f",
                    "ds_add_rtn"):
            assert bad not in body, (name, bad)


def test_no_float_arithmetic(scene_asm):
    """The contract is integer work only: no float instruction, conversion or compare in any scene kernel."""
    for name, body in _bodies(scene_asm).items():
        assert not re.search(r"\bv_(?:add|sub|mul|fma|fmac|mac|mad|cmp\w*|cvt)_\w*f(?:16|32|64)\b", body), name


def test_the_instructions_the_design_rests_on(scene_asm):
    for name, body in _bodies(scene_asm).items():
        if "k_scene_measure" in name:
            assert "v_sad_u8" in body and "v_dot4_u32_u8" in body, name
            assert "ds_add_u32" in body, name  # the histogram columns in LDS
    apply_body = next(body for name, body in _bodies(scene_asm).items() if "k_scene_apply" in name)
    assert "global_store_dwordx4" in apply_body and "v_perm_b32" in apply_body
