"""The forward-backward block-matching mode (nus_bm_set_bidirectional) on the MI355X: vectors, SADs and flags equal
tests/_bm_bidir.py bit for bit (integer work: no tolerance anywhere), the backward field is the search of (B, A), the frames are
the oracle's warp of the yardstick's vectors, the stream entry point gives each pair the one-pair calls' bytes, off means off,
and on the scene the mode is for its frame is nearer the true mid-frame than the default's.  Every device output lives in a
conftest.guarded tensor and comes down through nus_download."""
import functools

import numpy as np
import pytest

import _blockmatch as bmref
import _bm_bidir as bidir
from conftest import guarded
from nu_scaler_amd.transfer import to_device as put, to_numpy as fetch

pytestmark = pytest.mark.gpu

ORDERS = [bmref.SCAN, bmref.CENTER]
# kind, w, h, block size, radius
SCENES = [("scene", 192, 128, 8, 16), ("scene", 192, 128, 32, 8), ("scene", 200, 72, 16, 16)]
NOISE = [("noise", 33, 17, 8, 8), ("noise", 200, 72, 8, 24), ("noise", 200, 72, 16, 16), ("noise", 7, 5, 8, 4), ("noise", 1, 1, 8, 1),
         ("noise", 64, 48, 32, 8)]
CASES = SCENES + NOISE
_SCENE_ROW = {(192, 128, 8, 16): bidir.ROWS[0], (192, 128, 32, 8): bidir.ROWS[4], (200, 72, 16, 16): bidir.ROWS[5],
              (328, 200, 32, 8): (328, 200, 32, 8, (-4, 2), (6, -4), 48)}


@functools.lru_cache(maxsize=None)
def _pair(kind, w, h, bs, R):
    """(a, b, true mid-frame or None); read-only."""
    if kind == "scene":
        row = _SCENE_ROW[(w, h, bs, R)]
        out = bidir.scene(w, h, row[4], row[5], row[6])
    else:
        rng = np.random.default_rng(5)  # unrelated noise, A then B
        out = (rng.integers(0, 256, (h, w, 4), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8), None)
    for x in out:
        if x is not None:
            x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(kind, w, h, bs, R, order):
    """The yardstick's F, G, SADs, V and flags of the pair.  Computed once; read-only."""
    a, b, _ = _pair(kind, w, h, bs, R)
    e = bidir.estimate(a, b, bs, R, order)
    for x in e.values():
        x.setflags(write=False)
    return e


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _estimate(bm, a, b, sad=True, flags=True):
    """a, b: (n, h, w, 4) host -> (vectors, sad or None, flags or None) as numpy, from guarded tensors."""
    import torch

    n, h, w = a.shape[:3]
    da, db = put(np.ascontiguousarray(a)), put(np.ascontiguousarray(b))
    nbx, nby = bm.block_grid(w, h)
    ws_bytes = bm.workspace_size(w, h, n)
    ws = guarded.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    vec = guarded.empty((n, nby, nbx, 2), dtype=torch.int16, device="cuda:0")
    d_sad = guarded.empty((n, nby, nbx), dtype=torch.int32, device="cuda:0") if sad else None
    d_flags = guarded.empty((n, nby, nbx), dtype=torch.uint8, device="cuda:0") if flags else None
    fb = w * h * 4
    bm.estimate_device(da.data_ptr(), fb, db.data_ptr(), fb, w, h, n, ws.data_ptr(), ws_bytes, vec.data_ptr(),
                       d_sad.data_ptr() if sad else 0, d_flags.data_ptr() if flags else 0, 0, "f32", _stream())
    assert np.array_equal(fetch(da), a) and np.array_equal(fetch(db), b), "the input frames were written"
    return fetch(vec), (fetch(d_sad).view(np.uint32) if sad else None), (fetch(d_flags) if flags else None)


def _host_frames(bm, a, b, times, mode):
    h, w = a.shape[:2]
    return np.stack([np.frombuffer(x, np.uint8).reshape(h, w, 4) for x in bm.interpolate(a, b, w, h, times=times, mode=mode)])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind,w,h,bs,R", CASES)
def test_vectors_sads_and_flags_equal_the_yardstick(nsc, kind, w, h, bs, R, order):
    a, b, _ = _pair(kind, w, h, bs, R)
    e = _expected(kind, w, h, bs, R, order)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R, tie_order=order, bidirectional=True)
    v, s, f = _estimate(bm, a[None], b[None])
    print(f"{kind} {w}x{h} {bs}/{R} {order}: flags 4/8/16 on {[int((e['flags'] == k).sum()) for k in (4, 8, 16)]} of {e['flags'].size}")
    assert np.array_equal(s[0], e["sad_f"]), "sad"
    assert np.array_equal(f[0], e["flags"]), "flags"
    assert np.array_equal(v[0], e["V"]), "vectors"
    v2, none_s, none_f = _estimate(bm, a[None], b[None], sad=False, flags=False)  # the forward SADs live in the workspace then
    assert none_s is None and none_f is None and np.array_equal(v2, v)
    hv, hs, hf = bm.estimate(a, b, w, h)  # the host entry point
    assert np.array_equal(hv, e["V"]) and np.array_equal(hs, e["sad_f"]) and np.array_equal(hf, e["flags"])


def test_the_inputs_contain_every_kind_of_block():
    seen = set()
    for kind, w, h, bs, R in CASES:
        for order in ORDERS:
            seen |= set(_expected(kind, w, h, bs, R, order)["flags"].ravel().tolist())
    assert seen == {0, 4, 8, 16}, seen
    e = _expected("noise", 33, 17, 8, 8, bmref.CENTER)["flags"]
    assert [int((e == k).sum()) for k in (4, 8, 16)] == [1, 9, 4] and e.size == 15
    e = _expected("noise", 200, 72, 8, 24, bmref.CENTER)["flags"]
    assert [int((e == k).sum()) for k in (4, 8, 16)] == [12, 95, 106] and e.size == 225
    for w, h, bs, R in ((7, 5, 8, 4), (1, 1, 8, 1)):  # a single block, nothing admitted
        e = _expected("noise", w, h, bs, R, bmref.CENTER)
        assert e["flags"].tolist() == [[16]] and e["sad_f"][0, 0] == bidir.NO_MATCH


@pytest.mark.parametrize("order", ORDERS)
def test_pairs_of_a_batch_keep_their_own_fields(nsc, order):
    w, h, bs, R = 200, 72, 16, 16
    pairs = [_pair("scene", w, h, bs, R), _pair("noise", w, h, bs, R)]
    want = [_expected("scene", w, h, bs, R, order), _expected("noise", w, h, bs, R, order)]
    a, b = np.stack([p[0] for p in pairs] + [pairs[0][0]]), np.stack([p[1] for p in pairs] + [pairs[0][1]])
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R, tie_order=order, bidirectional=True)
    v, s, f = _estimate(bm, a, b)
    for k, e in enumerate(want + [want[0]]):
        assert np.array_equal(v[k], e["V"]) and np.array_equal(s[k], e["sad_f"]) and np.array_equal(f[k], e["flags"]), k


@pytest.mark.parametrize("kind,w,h,bs,R", [SCENES[0], SCENES[2], NOISE[0], NOISE[2]])
def test_the_backward_field_is_the_search_of_b_in_a(nsc, kind, w, h, bs, R):
    a, b, _ = _pair(kind, w, h, bs, R)
    e = _expected(kind, w, h, bs, R, bmref.CENTER)
    plain = nsc.BlockMatcher(block_size=bs, search_radius=R, refine=False)  # a second handle: mode off, refine off
    F, sad_f, flags_f = _estimate(plain, a[None], b[None])
    G, sad_g, _ = _estimate(plain, b[None], a[None])
    assert not flags_f.any()
    assert np.array_equal(F[0], e["F"]) and np.array_equal(G[0], e["G"]) and np.array_equal(sad_g[0], e["sad_g"])
    on = nsc.BlockMatcher(block_size=bs, search_radius=R, bidirectional=True)
    V, sad_v, flags = _estimate(on, a[None], b[None])
    want_v, want_flags = bidir.repair(F[0], sad_f[0], G[0], sad_g[0], w, h, bs)
    assert np.array_equal(V[0], want_v) and np.array_equal(flags[0], want_flags) and np.array_equal(sad_v, sad_f)
    for tol in (0, 4, 96):
        on.set_bidirectional(True, tol)
        V, _, flags = _estimate(on, a[None], b[None])
        want_v, want_flags = bidir.repair(F[0], sad_f[0], G[0], sad_g[0], w, h, bs, tol)
        assert np.array_equal(V[0], want_v) and np.array_equal(flags[0], want_flags), tol


def _fma_contract(got, want, share):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print(f"fma: max |diff| {d.max()}, bytes differing {(d != 0).sum()} of {d.size} ({(d != 0).mean():.5%})")
    assert d.max() <= 1, d.max()
    if share:  # the cap is defined on frames of at least 328 x 200
        assert (d != 0).sum() < 0.001 * d.size, (d != 0).mean()


@pytest.mark.parametrize("w,h,bs,R", [(192, 128, 8, 16), (200, 72, 16, 16), (328, 200, 32, 8)])
def test_frames_are_the_oracles_warp_of_the_yardstick_vectors(nsc, oracle_mod, w, h, bs, R):
    a, b, _ = _pair("scene", w, h, bs, R)
    V = _expected("scene", w, h, bs, R, bmref.CENTER)["V"]
    flow = bmref.dense_flow(V, w, h, bs)
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R, bidirectional=True)
    for m in (2, 4):
        times = nsc.frame_times(m)
        exact = _host_frames(bm, a, b, times, "exact")
        fma = _host_frames(bm, a, b, times, "fma")
        for j, t in enumerate(times):
            want = oracle_mod.warp_blend(a, b, flow, t)
            assert np.array_equal(exact[j], want), (m, j)
            _fma_contract(fma[j], want, (w, h) == (328, 200))


@functools.lru_cache(maxsize=None)
def _stream_frames():
    """(4, 72, 200, 4): the scene's A and B, then the noise pair: pair 0 is the scene, pairs 1 and 2 unrelated content."""
    a, b, _ = _pair("scene", 200, 72, 16, 16)
    na, nb, _ = _pair("noise", 200, 72, 16, 16)
    f = np.stack([a, b, na, nb])
    f.setflags(write=False)
    return f


def _run_stream(bm, frames, times, mode, vectors=True, frame_gap=0, mid_gap=0):
    """-> (mid (n_pairs, n_times, h, w, 4), vectors or None) from guarded tensors; the gaps of both strides are poisoned and checked."""
    import torch

    n, h, w = frames.shape[:3]
    n_pairs, fb, K = n - 1, w * h * 4, len(times)
    stride, mid_stride = fb + frame_gap, K * fb + mid_gap
    buf = np.full((n, stride), 0xEE, np.uint8)
    buf[:, :fb] = frames.reshape(n, fb)
    d_frames = put(buf)
    ws_bytes = bm.stream_workspace_size(w, h, n)
    ws = guarded.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    nbx, nby = bm.block_grid(w, h)
    vec = guarded.empty((n_pairs, nby, nbx, 2), dtype=torch.int16, device="cuda:0") if vectors else None
    mid = guarded.full((n_pairs, mid_stride), 0x5C, dtype=torch.uint8, device="cuda:0")
    bm.interpolate_stream_device(d_frames.data_ptr(), stride, n, w, h, ws.data_ptr(), ws_bytes, mid.data_ptr(), times=times, mode=mode,
                                 d_vectors=vec.data_ptr() if vectors else 0, mid_pair_stride=mid_stride if mid_gap else 0,
                                 stream=_stream())
    got = fetch(mid)
    assert (got[:, K * fb:] == 0x5C).all(), "the gap between the pairs' frames was written"
    assert np.array_equal(fetch(d_frames), buf), "the input stream or the gap between its frames was written"
    return got[:, :K * fb].reshape(n_pairs, K, h, w, 4), (fetch(vec) if vectors else None)


def test_stream_pairs_equal_the_one_pair_calls(nsc):
    w, h, bs, R = 200, 72, 16, 16
    frames = _stream_frames()
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R, bidirectional=True)
    times = nsc.frame_times(4)
    assert np.array_equal(bm.estimate(frames[0], frames[1], w, h)[0], _expected("scene", w, h, bs, R, bmref.CENTER)["V"])
    assert np.array_equal(bm.estimate(frames[2], frames[3], w, h)[0], _expected("noise", w, h, bs, R, bmref.CENTER)["V"])
    for mode in ("exact", "fma"):
        packed, vec = _run_stream(bm, frames, times, mode)
        gapped, gvec = _run_stream(bm, frames, times, mode, frame_gap=4 * 37, mid_gap=4 * 11)
        without, none = _run_stream(bm, frames, times, mode, vectors=False, frame_gap=4 * 5)  # the vectors live in the workspace
        assert np.array_equal(gapped, packed) and np.array_equal(gvec, vec) and none is None and np.array_equal(without, packed), mode
        for k in range(3):
            assert np.array_equal(vec[k], bm.estimate(frames[k], frames[k + 1], w, h)[0]), (mode, k)
            if mode == "exact":
                assert np.array_equal(packed[k], _host_frames(bm, frames[k], frames[k + 1], times, mode)), k
            else:
                for j in range(len(times)):
                    _fma_contract(packed[k, j], _host_frames(bm, frames[k], frames[k + 1], [times[j]], "exact")[0], False)


def test_off_means_off_and_refine_is_not_looked_at(nsc):
    w, h, bs, R = 200, 72, 16, 16
    a, b, _ = _pair("scene", w, h, bs, R)
    frames = _stream_frames()
    times = nsc.frame_times(2)

    def everything(bm):
        v, s, f = _estimate(bm, a[None], b[None])
        mid, vec = _run_stream(bm, frames, times, "exact")
        return [v, s, f, _host_frames(bm, a, b, times, "exact"), _host_frames(bm, a, b, times, "fma"), mid, vec]

    never = nsc.BlockMatcher(block_size=bs, search_radius=R)
    want = everything(never)
    assert (want[2] & 0x1C).sum() == 0 and (want[2] & 2).all(), "the default's flags: bits 0 and 1 only, the scene's motion is not smooth"
    bm = nsc.BlockMatcher(block_size=bs, search_radius=R)
    bm.set_bidirectional(True)
    on = everything(bm)
    assert not np.array_equal(on[0], want[0]) and (on[2] & 3).sum() == 0, "bits 0 and 1 stay clear with the mode on"
    bm.set_refine(False)
    for x, y in zip(everything(bm), on):
        assert np.array_equal(x, y), "set_refine(0) changed a byte with the mode on"
    bm.set_refine(True)
    for x, y in zip(everything(bm), on):
        assert np.array_equal(x, y), "set_refine(1) changed a byte with the mode on"
    bm.set_bidirectional(False)
    for k, (x, y) in enumerate(zip(everything(bm), want)):
        assert np.array_equal(x, y), f"output {k} of a handle turned on, used and turned off differs from a handle never turned on"


def test_quality_on_the_device(nsc):
    w, h, bs, R = 192, 128, 8, 16  # row 1 of the table
    a, b, mid = _pair("scene", w, h, bs, R)
    default = _host_frames(nsc.BlockMatcher(block_size=bs, search_radius=R), a, b, [0.5], "exact")[0]
    fb = _host_frames(nsc.BlockMatcher(block_size=bs, search_radius=R, bidirectional=True), a, b, [0.5], "exact")[0]
    p_default, p_fb = bidir.psnr_rgb(default, mid), bidir.psnr_rgb(fb, mid)
    print(f"PSNR against the true mid-frame: default {p_default:.2f} dB, forward-backward {p_fb:.2f} dB")
    assert p_fb >= p_default + 1.0
    it = nsc.PyFrameInterpolator("block_matching", "high", bidirectional=True)
    it.initialize(w, h)
    high = nsc.BlockMatcher("high", bidirectional=True)
    assert it.interpolate(a, b, 0.5) == high.interpolate(a, b, w, h, times=[0.5])[0]
