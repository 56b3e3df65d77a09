"""The FMA-mode six-tap x2 kernels exchange the horizontal pass's halo columns through LDS (lanczos_x2_hpass,
nus_k_lanczos_x2.hip) where the commit before exchanged them with DPP moves.  The tap order of every sum is unchanged, so every
output byte must be what that commit wrote: tests/golden/x2_fma_parent_digests.json holds the SHA-256 digests of every output
buffer tools/x2_output_digests.py recorded there (on the GPU, same script, same numpy default_rng inputs); no tolerance."""
import json
import os
import sys

import pytest
from conftest import GOLDEN, ROOT, guarded

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "x2_fma_parent_digests.json")) as fh:
        doc = json.load(fh)
    assert len(doc["commit"]) == 40 and "default_rng" in doc["recipe"]
    return doc["digests"]


def test_every_recorded_case_is_run(parent):
    import x2_output_digests as dig

    assert sorted(parent) == sorted(f"{w}x{h}/rows_per_wave{th}" for w, h in dig.SHAPES for th in dig.ROWS_PER_WAVE)
    assert dig.SHAPES == [(16, 16), (244, 19), (484, 37), (724, 23)] and dig.ROWS_PER_WAVE == [0, 6] and dig.N_UNITS == 3
    for case in parent.values():  # 3 contents x (upscale + 2 blends + 2 units x 3 buffers) + the variant's name
        assert len(case) == 3 * (1 + 2 + 2 * 3) + 1


@pytest.mark.parametrize("th", [0, 6])
@pytest.mark.parametrize("w,h", [(16, 16), (244, 19), (484, 37), (724, 23)])
def test_outputs_are_the_parent_commits(nsc, parent, w, h, th):
    """upscale_device, upscale_blend_device (t = 0.5, 0.3) and upscale_unit_device (t = 0.5, 0.3; all three outputs) on opaque
    noise, 4-channel noise and a frame whose alpha is flat 255, flat 128 or noisy in bands of 5 rows (the 3- and 4-channel paths,
    12- and 16-plane writes, alternate inside a tap window): 3 frames per launch, digest for digest what the parent recorded."""
    import x2_output_digests as dig

    want = parent[f"{w}x{h}/rows_per_wave{th}"]
    got = dig.run_shape(w, h, th, zeros=guarded.zeros)
    assert got["kernel_variant"] == want["kernel_variant"] == "lanczos3_x2_regwin"
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert differ == [], (w, h, th, differ)


def _unit(u, torch, frames, w, h, n, t):
    fb = w * h * 4
    mid = guarded.zeros((n, h, w, 4), dtype=torch.uint8, device=frames.device)
    up_real = guarded.zeros((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device=frames.device)
    up_mid = guarded.zeros_like(up_real)
    u.upscale_unit_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, t, mid.data_ptr(), up_real.data_ptr(), up_mid.data_ptr(), n,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return mid, up_real, up_mid


@pytest.mark.parametrize("t", [0.5, 0.3])
def test_unit_step_equals_the_three_stages_and_repeats(nsc, t):
    """484 x 37, three strips: the one-launch step bit for bit the three stages (blend, upscale, upscale), and two consecutive
    runs on the same input bit for bit each other -- the four waves of a block each own an exchange area in LDS, and waves that
    read each other's would differ from run to run."""
    import torch
    import x2_output_digests as dig
    from nu_scaler_amd.transfer import to_device as put

    w, h, n = 484, 37, dig.N_UNITS
    fb = w * h * 4
    s = torch.cuda.current_stream().cuda_stream
    for content in dig.CONTENTS:
        frames = put(dig.make_frames(w, h, content))
        for th in (0, 6):
            u = nsc.PyWgpuUpscaler("quality", "lanczos3")
            if th:
                u.set_option("rows_per_wave", th)
            u.initialize(w, h, 2 * w, 2 * h)
            first = _unit(u, torch, frames, w, h, n, t)
            second = _unit(u, torch, frames, w, h, n, t)
            want_mid = guarded.zeros((n, h, w, 4), dtype=torch.uint8, device=frames.device)
            want_real = guarded.zeros((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device=frames.device)
            want_up_mid = guarded.zeros_like(want_real)
            nsc.WgpuFrameInterpolator().interpolate_device(frames.data_ptr(), fb, frames.data_ptr() + fb, fb, 0, w, h, t,
                                                           want_mid.data_ptr(), n, s)
            u.upscale_device(frames.data_ptr(), want_real.data_ptr(), n, s)
            u.upscale_device(want_mid.data_ptr(), want_up_mid.data_ptr(), n, s)
            torch.cuda.synchronize()
            for name, a, b, c in zip(("mid", "up_real", "up_mid"), first, second, (want_mid, want_real, want_up_mid)):
                assert torch.equal(a, b), ("two runs differ", name, content, th, t)
                assert torch.equal(a, c), ("unit step != three stages", name, content, th, t)
