"""The rate conversion behind the two motion estimators, on the MI355X.  nus_flow_retime_device_stream equals
nus_flow_estimate_device_stream followed by nus_interp_retime_device in FMA mode, byte for byte, in both estimator modes, with and
without re-linearisation, and with a chunk edge inside the schedule; nus_bm_retime_device_stream in EXACT mode equals
nus_bm_interpolate pair by pair and copies at the real frames; with scene detection on, a cut pair's in-between outputs are repeats
of the nearer frame and every other output is unchanged; the Python wrappers and PyFrameInterpolator.retime return the same bytes.
The estimator stream and the scene-detecting streams run at 67 x 45 and at 66 x 44: the even width and the pixel count on a
multiple of 4 select the pixel-pair and the 16-byte kernels.  Every device output comes from conftest.guarded."""
import os

import numpy as np
import pytest

import _flow_warp64
import _retime
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

W, H, N = 67, 45, 5
FB = W * H * 4
EVEN = (66, 44)  # beside the odd width: the XV = 2 tile kernels and, with w*h % 4 == 0, the 16-byte streaming kernels
RATIOS = [(5, 2), (2, 5)]
POISON = 0x3C


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def lattice():
    frames = _flow_warp64.lattice_frames(W, H, N)
    frames.setflags(write=False)
    return frames


@pytest.fixture(scope="module")
def lattice_even():
    frames = _flow_warp64.lattice_frames(*EVEN, N)
    frames.setflags(write=False)
    return frames


def _out(n_out, w=W, h=H):
    import torch

    return guarded.full((n_out, h, w, 4), POISON, dtype=torch.uint8, device="cuda:0")


@pytest.mark.parametrize("chunk", [None, "2"])
@pytest.mark.parametrize("warps", [0, 1])
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_flow_stream_equals_estimate_then_retime_warp(nsc, lattice, lattice_even, mode, warps, chunk):
    """At 67 x 45 and at 66 x 44; at the even width the only test in which the estimator's route (StreamJob chunks with their
    first_pair) launches the pixel-pair kernel k_retime_flow_proj<Fma, f32, XV = 2> and the 16-byte k_retime_real<true>."""
    for size, frames in (((W, H), lattice), (EVEN, lattice_even)):
        assert (size[0] % 2 == 0 and size[0] * size[1] % 4 == 0) == (size == EVEN)
        _flow_stream_case(nsc, frames, size, mode, warps, chunk)


def _flow_stream_case(nsc, frames, size, mode, warps, chunk):
    import torch

    W, H = size
    FB = W * H * 4
    d_frames = put(frames)
    fe = nsc.FlowEstimator(warps=warps)
    fe.set_mode(mode)
    fe.set_project(1)
    it = nsc.WgpuFrameInterpolator()
    it.set_mode("fma")
    it.set_flow_project(1)
    old = os.environ.pop("NUS_FLOW_MAX_CHUNK_PAIRS", None)
    try:
        if chunk is not None:
            os.environ["NUS_FLOW_MAX_CHUNK_PAIRS"] = chunk  # a chunk edge inside the schedule
        for num, den in RATIOS:
            n_out = _retime.count(N, num, den)
            flows_a = guarded.empty((N - 1, H, W, 2), dtype=torch.float32, device="cuda:0")
            flows_b = guarded.empty((N - 1, H, W, 2), dtype=torch.float32, device="cuda:0")
            got, want = _out(n_out, W, H), _out(n_out, W, H)
            fe.retime_device_stream(d_frames.data_ptr(), N, W, H, num, den, got.data_ptr(), flows_a.data_ptr(), 0, _stream())
            fe.estimate_device_stream(d_frames.data_ptr(), N, W, H, flows_b.data_ptr(), _stream())
            it.retime_device(d_frames.data_ptr(), FB, N, flows_b.data_ptr(), W, H, num, den, want.data_ptr(), 0, _stream())
            assert np.array_equal(fetch(flows_a).view(np.uint32), fetch(flows_b).view(np.uint32)), (mode, warps, chunk, num, den)
            g, w_ = fetch(got), fetch(want)
            assert np.array_equal(g, w_), (mode, warps, chunk, num, den, [j for j in range(n_out) if not np.array_equal(g[j], w_[j])])
            # without d_flows the frames are the same
            again = _out(n_out, W, H)
            fe.retime_device_stream(d_frames.data_ptr(), N, W, H, num, den, again.data_ptr(), 0, 0, _stream())
            assert np.array_equal(fetch(again), g), (mode, warps, chunk, num, den, "no d_flows")
    finally:
        os.environ.pop("NUS_FLOW_MAX_CHUNK_PAIRS", None)
        if old is not None:
            os.environ["NUS_FLOW_MAX_CHUNK_PAIRS"] = old


def _bm_retime(bm, d_frames, n, num, den, mode="exact", w=W, h=H):
    import torch

    ws_bytes = bm.stream_workspace_size(w, h, n)
    ws = guarded.empty((ws_bytes + 16,), dtype=torch.uint8, device="cuda:0")
    d_ws = (ws.data_ptr() + 15) & ~15
    out = _out(_retime.count(n, num, den), w, h)
    bm.retime_stream_device(d_frames.data_ptr(), w * h * 4, n, w, h, num, den, d_ws, ws_bytes, out.data_ptr(), mode=mode, stream=_stream())
    return fetch(out)


@pytest.mark.parametrize("bidir", [False, True])
def test_block_matching_stream_equals_the_pairwise_host_entry(nsc, lattice, bidir):
    d_frames = put(lattice)
    bm = nsc.BlockMatcher("medium", bidirectional=bidir)
    for num, den in RATIOS:
        got = _bm_retime(bm, d_frames, N, num, den)
        for j, (k, r, t) in enumerate(_retime.schedule(N, num, den)):
            if r == 0:
                assert np.array_equal(got[j], lattice[k]), (bidir, num, den, j)
            else:
                want = np.frombuffer(bm.interpolate(lattice[k], lattice[k + 1], W, H, times=[float(t)], mode="exact")[0], np.uint8)
                assert np.array_equal(got[j].reshape(-1), want), (bidir, num, den, j, k, float(t))


def _cut_stream(lattice):
    frames = np.array(lattice)
    frames[3:] = frames[3:][..., ::-1, :] // 4  # from frame 3 on another, dark scene: pair (2, 3) is the one hard cut
    frames[..., 3] = 255
    return frames


@pytest.mark.parametrize("engine", ["flow", "bm"])
def test_scene_detection_repeats_the_nearer_frame_on_the_cut_pair_only(nsc, lattice, lattice_even, engine):
    """At 67 x 45 and at 66 x 44 (2904 px, a multiple of 4); at the latter the only test in which the detectors inside the two
    stream entry points hand their flags to k_retime_scene_apply<true>, behind k_retime_bm<Exact, XV = 2> / k_retime_flow_proj's
    pair form."""
    for size, frames in (((W, H), lattice), (EVEN, lattice_even)):
        assert (size[0] * size[1] % 4 == 0) == (size == EVEN)
        _scene_detection_case(nsc, frames, size, engine)


def _scene_detection_case(nsc, lattice, size, engine):
    import _scenecut as sc

    W, H = size
    frames = _cut_stream(lattice)
    cut = [bool(sc.is_cut(*sc.measures(frames[k], frames[k + 1]), W, H)) for k in range(N - 1)]
    assert cut == [False, False, True, False]
    d_frames = put(frames)
    h = nsc.FlowEstimator() if engine == "flow" else nsc.BlockMatcher("medium")

    def run(num, den):
        if engine == "bm":
            return _bm_retime(h, d_frames, N, num, den, w=W, h=H)
        out = _out(_retime.count(N, num, den), W, H)
        h.retime_device_stream(d_frames.data_ptr(), N, W, H, num, den, out.data_ptr(), 0, 0, _stream())
        return fetch(out)

    for num, den in RATIOS + [(3, 1)]:
        off = run(num, den)
        h.set_scene_detect(True)
        try:
            on = run(num, den)
        finally:
            h.set_scene_detect(False)
        touched = 0
        for j, (k, r, t) in enumerate(_retime.schedule(N, num, den)):
            if r != 0 and cut[k]:  # (a real frame, the stream's last one included, belongs to no pair)
                assert np.array_equal(on[j], frames[k] if float(t) < 0.5 else frames[k + 1]), (engine, num, den, j)
                touched += 1
            else:
                assert np.array_equal(on[j], off[j]), (engine, num, den, j)
        assert touched or (num, den) == (2, 5)
        assert np.array_equal(run(num, den), off), "with detection off again no byte differs"


def test_apply_cuts_entry_point_on_its_own(nsc, lattice):
    import torch

    d_frames = put(lattice)
    lib = nsc._capi.lib()
    num, den = 12, 5
    n_out = _retime.count(N, num, den)
    for fmt, name in ((0, "rgba"), (1, "bgra"), (3, "bgrx")):
        out = _out(n_out)
        d_cut = put(np.array([0, 1, 0, 1], np.uint8))
        assert lib.nus_scene_apply_cuts_retime_device(d_frames.data_ptr(), FB, N, W, H, fmt, num, den, d_cut.data_ptr(), out.data_ptr(), 0,
                                                      _stream()) == 0, nsc._capi.last_error()
        got = fetch(out)
        it = nsc.WgpuFrameInterpolator()
        it.set_input_format(name)
        for j, (k, r, t) in enumerate(_retime.schedule(N, num, den)):
            if k in (1, 3) and r != 0:  # the copy: the zero-flow call at t = 0 / 1
                ref = guarded.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
                base = d_frames.data_ptr() + k * FB
                it.interpolate_device(base, FB, base + FB, FB, 0, W, H, 0.0 if float(t) < 0.5 else 1.0, ref.data_ptr(), 1, _stream())
                assert np.array_equal(got[j], fetch(ref)), (name, j)
            else:
                assert (got[j] == POISON).all(), (name, j, "an output of a pair that is not cut, or a real frame, was written")


@pytest.mark.parametrize("method", ["optical_flow", "block_matching"])
def test_host_frame_retime_returns_the_device_bytes(nsc, lattice, method):
    import torch

    num, den = 5, 2
    pi = nsc.PyFrameInterpolator(method, "medium")
    pi.initialize(W, H)
    got = pi.retime([f.tobytes() for f in lattice[:4]], 24, 60)
    sched = _retime.schedule(4, num, den)
    assert len(got) == len(sched) and all(len(g) == FB for g in got)
    for j, (k, r, t) in enumerate(sched):
        want = lattice[k].tobytes() if r == 0 else pi.interpolate(lattice[k].tobytes(), lattice[k + 1].tobytes(), float(t))
        assert got[j] == bytes(want), (method, j, k, r)
    assert pi.retime([f.tobytes() for f in lattice[:4]], 60, 150) == got  # the ratio is reduced
    with pytest.raises(ValueError):
        pi.retime([f.tobytes() for f in lattice[:4]], 1, 9)


@pytest.mark.parametrize("method", ["optical_flow", "block_matching"])
def test_host_frame_retime_with_scene_detection_equals_interpolate(nsc, lattice, method):
    frames = _cut_stream(lattice)  # pair (2, 3) is a cut
    pi = nsc.PyFrameInterpolator(method, "medium", scene_detect=True)
    pi.initialize(W, H)
    got = pi.retime([f.tobytes() for f in frames], 2, 5)
    sched = _retime.schedule(N, 5, 2)
    assert len(got) == len(sched)
    repeats = 0
    for j, (k, r, t) in enumerate(sched):
        want = frames[k].tobytes() if r == 0 else pi.interpolate(frames[k].tobytes(), frames[k + 1].tobytes(), float(t))
        assert got[j] == bytes(want), (method, j, k, r)
        if r != 0 and k == 2:
            assert got[j] == (frames[2] if float(t) < 0.5 else frames[3]).tobytes(), (method, j)
            repeats += 1
    assert repeats == 2


def _write_inputs(tmp_path, frames):
    from nu_scaler_amd.imagefile import write_png

    paths = []
    for k, f in enumerate(frames):
        paths.append(str(tmp_path / f"in{k}.png"))
        write_png(paths[-1], W, H, f.tobytes())
    return paths


def _run_cli(argv, args, tmp_path):
    import subprocess

    from conftest import ROOT

    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(argv + ["retime"] + args, capture_output=True, text=True, cwd=tmp_path, env=env, timeout=300)
    assert r.returncode == 0, (argv, args, r.stdout, r.stderr)
    return r.stdout.split()


def _native(nsc):
    return [os.path.join(os.path.dirname(os.path.dirname(nsc._capi.LIB_PATH)), "bin", "nu_scaler_cli")]


def test_both_clis_write_the_same_pngs(nsc, lattice, tmp_path):
    """The 4-frame, 5/2 case: `python -m nu_scaler_amd.cli retime` (the device-resident conversion) and the native tool (one host
    call per pair from nus_retime_schedule) write the same 8 PNGs, and they are the frames of the schedule."""
    import sys

    from _png import read_png

    inputs = _write_inputs(tmp_path, lattice[:4])
    py = _run_cli([sys.executable, "-m", "nu_scaler_amd.cli"], ["--from", "24", "--to", "60", "py_%04d.png"] + inputs, tmp_path)
    nat = _run_cli(_native(nsc), ["--from", "24", "--to", "60", "nat_%04d.png"] + inputs, tmp_path)
    sched = _retime.schedule(4, 5, 2)
    assert py == [f"py_{j:04d}.png" for j in range(len(sched))] and nat == [f"nat_{j:04d}.png" for j in range(len(sched))]
    pi = nsc.PyFrameInterpolator("optical_flow")
    pi.initialize(W, H)
    for j, (k, r, t) in enumerate(sched):
        a, b = read_png(str(tmp_path / py[j])), read_png(str(tmp_path / nat[j]))
        assert np.array_equal(a, b), j
        want = lattice[k] if r == 0 else np.frombuffer(pi.interpolate(lattice[k].tobytes(), lattice[k + 1].tobytes(), float(t)), np.uint8)
        assert np.array_equal(a.reshape(-1), np.asarray(want).reshape(-1)), j


@pytest.mark.parametrize("flags", [["--method", "blend", "--scene-detect"],
                                   ["--method", "block_matching", "--bidirectional", "--scene-detect"],
                                   ["--method", "optical_flow", "--flow-warps", "1", "--flow-median", "3", "--flow-project", "2"]])
def test_native_cli_equals_the_package_for_every_method(nsc, lattice, tmp_path, flags):
    """The other methods and flags, the package side in this process (nu_scaler_amd.cli.main): a cut stream at 12/5 and a fraction."""
    from _png import read_png
    from nu_scaler_amd import cli

    inputs = _write_inputs(tmp_path, _cut_stream(lattice))
    rates = ["--from", "25", "--to", "60"]
    nat = _run_cli(_native(nsc), rates + flags + ["nat_%d.png"] + inputs, tmp_path)
    assert cli.main(["retime"] + rates + flags + [str(tmp_path / "py_%d.png")] + inputs) == 0
    assert len(nat) == _retime.count(N, 12, 5)
    for j in range(len(nat)):
        assert np.array_equal(read_png(str(tmp_path / f"py_{j}.png")), read_png(str(tmp_path / nat[j]))), (flags, j)
