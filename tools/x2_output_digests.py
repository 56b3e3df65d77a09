#!/usr/bin/env python
"""SHA-256 digests of every output buffer of the FMA-mode x2 Lanczos-3 entry points on a set of small frames (dev tool and test
helper).  Only the public Python API is used, so the script runs unchanged on a checkout of an older commit: run there once,

    python tools/x2_output_digests.py --commit <id of that commit> -o tests/golden/x2_fma_parent_digests.json

its digests are what tests/test_x2_lane_exchange.py holds a later build to, bit for bit.  The inputs are numpy default_rng
streams; the recipe (RECIPE, below) is recorded next to the digests."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

# w x h: one strip (the minimum the variant accepts); two strips, the second 4 columns wide; three strips; four strips
SHAPES = [(16, 16), (244, 19), (484, 37), (724, 23)]
ROWS_PER_WAVE = [0, 6]  # 6: several row blocks and a short last one
CONTENTS = ["opaque", "noise4", "bands"]
N_UNITS = 3
BLEND_T = [0.5, 0.3]
RECIPE = ("frames = numpy.random.default_rng(seed).integers(0, 256, (N_UNITS + 1, h, w, 4), dtype=uint8), "
          "seed = 10 * w + index of the content in CONTENTS; opaque: alpha = 255; noise4: as drawn; bands: rows in bands of 5, "
          "band b of every frame has alpha 255 (b % 3 == 0), 128 (b % 3 == 1) or as drawn (b % 3 == 2)")


def make_frames(w, h, content):
    rng = np.random.default_rng(10 * w + CONTENTS.index(content))
    f = rng.integers(0, 256, (N_UNITS + 1, h, w, 4), dtype=np.uint8)
    if content == "opaque":
        f[..., 3] = 255
    elif content == "bands":
        for b in range((h + 4) // 5):
            if b % 3 == 0:
                f[:, 5 * b:5 * b + 5, :, 3] = 255
            elif b % 3 == 1:
                f[:, 5 * b:5 * b + 5, :, 3] = 128
    return f


def _sha(t):
    from nu_scaler_amd.transfer import to_numpy

    return hashlib.sha256(np.ascontiguousarray(to_numpy(t)).tobytes()).hexdigest()


def run_shape(w, h, th, zeros=None):
    """{"<content>/<entry point>/<buffer>": digest} for one frame size and rows_per_wave.  zeros(shape, dtype=, device=)
    allocates the zero-filled device outputs (default torch.zeros)."""
    import torch

    import nu_scaler_amd as nsc
    from nu_scaler_amd.transfer import to_device

    zeros = zeros or torch.zeros
    dev = torch.device("cuda:0")
    n, fb = N_UNITS, w * h * 4
    s = torch.cuda.current_stream().cuda_stream
    u = nsc.PyWgpuUpscaler("quality", "lanczos3")  # lanczos_mode "fma" is the default
    if th:
        u.set_option("rows_per_wave", th)
    u.initialize(w, h, 2 * w, 2 * h)
    out = {"kernel_variant": u.kernel_variant}
    for content in CONTENTS:
        frames = to_device(make_frames(w, h, content), "cuda:0")
        a, b = frames.data_ptr(), frames.data_ptr() + fb

        def big():
            return zeros((n, 2 * h, 2 * w, 4), dtype=torch.uint8, device=dev)

        up = big()
        u.upscale_device(a, up.data_ptr(), n, s)
        torch.cuda.synchronize()
        out[f"{content}/upscale/out"] = _sha(up)
        for t in BLEND_T:
            up = big()
            u.upscale_blend_device(a, fb, b, fb, t, up.data_ptr(), n, s)
            torch.cuda.synchronize()
            out[f"{content}/blend_t{t}/out"] = _sha(up)
            mid, up_real, up_mid = zeros((n, h, w, 4), dtype=torch.uint8, device=dev), big(), big()
            u.upscale_unit_device(a, fb, b, fb, t, mid.data_ptr(), up_real.data_ptr(), up_mid.data_ptr(), n, s)
            torch.cuda.synchronize()
            out[f"{content}/unit_t{t}/mid"] = _sha(mid)
            out[f"{content}/unit_t{t}/out_real"] = _sha(up_real)
            out[f"{content}/unit_t{t}/out_mid"] = _sha(up_mid)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="id of the commit this checkout is at (recorded with the digests)")
    ap.add_argument("-o", "--out", required=True)
    a = ap.parse_args()
    doc = {"commit": a.commit, "recipe": RECIPE, "n_units": N_UNITS, "digests": {}}
    for w, h in SHAPES:
        for th in ROWS_PER_WAVE:
            doc["digests"][f"{w}x{h}/rows_per_wave{th}"] = run_shape(w, h, th)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{sum(len(v) - 1 for v in doc['digests'].values())} digests -> {a.out}")


if __name__ == "__main__":
    main()
