"""bench.py's plain run and --dump-outputs: what the last timed step computed, written as float32 .npy files (whole, or a fixed
seeded sample of a large output), and a plain run that leaves every leg of --full out of its line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_plain_run_is_the_default_and_full_is_an_option():
    bench = _bench()
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_positions_are_fixed_sorted_and_in_bounds():
    bench = _bench()
    assert bench.dump_positions("up_real", 1000, 1000) is None
    p = bench.dump_positions("up_real", 10 ** 10, 4096)
    assert p.dtype == np.int64 and p.shape == (4096,) and np.all(np.diff(p) >= 0) and p[0] >= 0 and p[-1] < 10 ** 10
    assert np.array_equal(p, bench.dump_positions("up_real", 10 ** 10, 4096))
    assert not np.array_equal(p, bench.dump_positions("up_mid", 10 ** 10, 4096))


def test_dump_outputs_on_host_tensors(tmp_path):
    import torch

    bench = _bench()
    small = torch.arange(2 * 3 * 4, dtype=torch.uint8).view(2, 3, 4)
    big = (torch.arange(5000, dtype=torch.int64) % 251).to(torch.uint8).view(50, 100)
    written = bench.dump_outputs(str(tmp_path), [("small", small), ("big", big)], max_elements=1000)
    assert written == {"small": (24, 24), "big": (5000, 1000)}
    s, b = np.load(tmp_path / "small.npy"), np.load(tmp_path / "big.npy")
    assert s.dtype == np.float32 and np.array_equal(s, np.arange(24, dtype=np.float32))
    assert b.dtype == np.float32 and np.array_equal(b, (bench.dump_positions("big", 5000, 1000) % 251).astype(np.float32))
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path), [("strided", big[:, ::2])])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(nsc, oracle_mod, tmp_path):
    """A plain run: one JSON line with the headline fields and none of --full's legs; the dumped outputs are the oracle's
    (in-between frames bit-exact; both upscaled frames within 1 LSB, < 0.1 % of samples differing)."""
    w, h, n = 496, 270, 5
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--units", str(n), "--width", str(w), "--height", str(h),
           "--steps", "4", "--warmup", "1", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), lines[:4]
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["dtype"] and d["metric"]
    assert abs(d["ms_per_step"] - d["config"]["timed_region_s"] * 1e3 / 4) < 0.13  # (timed_region_s is rounded to 1 ms)
    c = d["config"]
    assert c["full"] is False and "cpu_baseline" not in d
    assert c["per_rank_check"] is None and c["sustained"] is None and c["host_path"] is None and c["host_fed"] is None
    assert c["motion_variant"] is None and (d["roofline"] is None or d["roofline"]["traffic"] is None)

    bench = _bench()
    src = [oracle_mod.gen_gradient(w, h, k) for k in range(n + 1)]
    mids = np.stack([oracle_mod.warp_blend(src[k], src[k + 1], None, 0.5) for k in range(n)])
    ups = {"up_real": np.stack([oracle_mod.lanczos3(src[k], 2 * w, 2 * h, threads=0) for k in range(n)]),
           "up_mid": np.stack([oracle_mod.lanczos3(m, 2 * w, 2 * h, threads=0) for m in mids])}
    got = np.load(out / "mid.npy")
    assert got.dtype == np.float32 and bench.dump_positions("mid", mids.size) is None
    assert np.array_equal(got, mids.reshape(-1).astype(np.float32))
    for name, want in ups.items():
        got = np.load(out / f"{name}.npy")
        pos = bench.dump_positions(name, want.size)
        assert got.dtype == np.float32 and pos is not None and got.shape == pos.shape
        diff = np.abs(got - want.reshape(-1)[pos].astype(np.float32))
        assert diff.max() <= 1 and (diff > 0).mean() < 1e-3, name
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 * 10 ** 6
