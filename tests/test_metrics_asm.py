"""The metrics kernels (nus_k_metrics.hip) as hipcc builds them for gfx950, checked without a GPU: no scratch (register
spills would sit on the SSIM kernel's VALU-bound path) and no float atomics or compare-and-swap loops (the determinism rule:
partials go to the workspace and are added in a fixed order)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")
KERNELS = ("k_metrics_sse", "k_metrics_ssim", "k_metrics_finish")


@pytest.fixture(scope="module")
def metrics_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("asm") / "nus_k_metrics.s"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
           "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out),
           os.path.join(CSRC, "nus_k_metrics.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return out.read_text()


def _bodies(asm):
    """{mangled kernel name: its instruction text} for every metrics kernel."""
    out = {}
    for m in re.finditer(r"^(_Z\S*(?:%s)\S*):" % "|".join(KERNELS), asm, re.M):
        name = m.group(1)
        end = asm.find(".Lfunc_end", m.end())
        out[name] = asm[m.end():end]
    return out


def test_built_with_the_makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-O3 -std=c++17 -fPIC -ffp-contract=off" in mk
    assert "nus_k_metrics.hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0]


def test_every_kernel_is_there(metrics_asm):
    names = list(_bodies(metrics_asm))
    for k in KERNELS:
        assert any(k in n for n in names), (k, names)
    assert sum("k_metrics_ssim" in n for n in names) == 2  # with and without the fused SSE
    assert all("s_endpgm" in body for body in _bodies(metrics_asm).values())


def test_no_scratch(metrics_asm):
    found = 0
    for m in re.finditer(r"^\s+\.name:\s+(\S+)\s*$", metrics_asm, re.M):
        name = m.group(1)
        if not any(k in name for k in KERNELS) or name.endswith(".kd"):
            continue
        block = metrics_asm[m.start():m.start() + 4000]
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        assert priv and int(priv.group(1)) == 0, (name, priv and priv.group(0))
        found += 1
    assert found >= 4
    for name, body in _bodies(metrics_asm).items():
        assert "scratch_" not in body and "buffer_store" not in body, name


def test_no_float_atomics_or_cmpswap(metrics_asm):
    for name, body in _bodies(metrics_asm).items():
        for bad in ("global_atomic_add_f32", "global_atomic_add_f64", "global_atomic_pk_add", "cmpswap", "flat_atomic"):
            assert bad not in body, (name, bad)
