"""Frame-rate conversion by a rational ratio (24 -> 60, 25 -> 60, 30 -> 144, 60 -> 24): the schedule of the library's retime
entry points (include/nuscaler_hip.h, "Frame-rate conversion by a rational ratio") mirrored in Python, and the library's own
table.  BUILD-DEFINED: the reference has no rate conversion.

With num / den = fps_out / fps_in reduced by its gcd, output j of a stream of n_frames frames is

    k_j = (j * den) // num,   r_j = (j * den) % num,   t_j = float32(r_j / num),   n_out = ((n_frames - 1) * num) // den + 1

r_j == 0: real frame k_j; else the in-between frame of pair (k_j, k_j + 1) at t_j.  The device wrappers are
`WgpuFrameInterpolator.retime_device`, `FlowEstimator.retime_device_stream` and `BlockMatcher.retime_stream_device`; host frames go
through `PyFrameInterpolator.retime`."""
from __future__ import annotations

import ctypes
from fractions import Fraction
from typing import NamedTuple

import numpy as np

from . import _capi as C


class RetimeEntry(NamedTuple):
    pair: int   # k_j
    rem: int    # r_j of the reduced ratio; 0: the output is real frame `pair`
    t: float    # t_j, a float32 value


class _Entry(ctypes.Structure):  # nus_retime_entry
    _fields_ = [("pair", ctypes.c_uint32), ("rem", ctypes.c_uint32), ("t", ctypes.c_float), ("reserved", ctypes.c_uint32)]


def retime_ratio(fps_in, fps_out) -> tuple[int, int]:
    """(num, den) = fps_out / fps_in reduced, from ints or Fractions (30000/1001 is Fraction(30000, 1001)); ValueError for what
    the library refuses: a rate that is not positive, a reduced term above RETIME_MAX_TERM, a ratio above INTERP_MAX_TIMES + 1."""
    for name, v in (("fps_in", fps_in), ("fps_out", fps_out)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer, Fraction)):
            raise ValueError(f"{name} must be an int or a Fraction, got {v!r}")
        if v <= 0:
            raise ValueError(f"{name} must be positive, got {v!r}")
    r = Fraction(fps_out) / Fraction(fps_in)
    num, den = r.numerator, r.denominator
    if num > C.RETIME_MAX_TERM or den > C.RETIME_MAX_TERM:
        raise ValueError(f"the reduced ratio {num}/{den} has a term above {C.RETIME_MAX_TERM}")
    if num > (C.INTERP_MAX_TIMES + 1) * den:
        raise ValueError(f"the ratio {num}/{den} is above {C.INTERP_MAX_TIMES + 1}")
    return num, den


def retime_count(n_frames: int, fps_in, fps_out) -> int:
    """Output frames of the conversion of `n_frames` >= 2 input frames."""
    num, den = retime_ratio(fps_in, fps_out)
    if int(n_frames) < 2:
        raise ValueError("a stream needs at least 2 frames")
    return ((int(n_frames) - 1) * num) // den + 1


def retime_schedule(n_frames: int, fps_in, fps_out) -> list[RetimeEntry]:
    """The schedule in Python integers and one float32 division per entry: what nus_retime_schedule returns."""
    num, den = retime_ratio(fps_in, fps_out)
    out = []
    for j in range(retime_count(n_frames, fps_in, fps_out)):
        k, r = divmod(j * den, num)
        out.append(RetimeEntry(k, r, float(np.float32(r) / np.float32(num))))
    return out


def library_schedule(n_frames: int, num: int, den: int, first: int = 0, count: int | None = None) -> list[RetimeEntry]:
    """nus_retime_schedule: entries first .. first + count - 1 (all from `first` on when count is None) of the library's own
    table, for the ratio as given (the library reduces it).  ValueError with the library's text for what it refuses."""
    lib = C.lib()
    n_out = int(lib.nus_retime_count(int(n_frames), int(num), int(den)))
    if n_out < 0:
        raise ValueError(C.last_error())
    cnt = max(n_out - int(first), 0) if count is None else int(count)
    buf = (_Entry * max(cnt, 1))()
    if lib.nus_retime_schedule(int(n_frames), int(num), int(den), int(first), cnt, ctypes.addressof(buf)) != C.OK:
        raise ValueError(C.last_error())
    return [RetimeEntry(int(buf[i].pair), int(buf[i].rem), float(buf[i].t)) for i in range(cnt)]


def retime_frames(frames, w: int, h: int, fps_in, fps_out, *, matcher=None, warp=None, flow=None, scene=None,
                  device: int = 0, select: bool = False) -> list[bytes]:
    """Host frames (w*h*4 bytes each) -> the host frames of the conversion, through the device entry points: one upload, then
    `matcher.retime_stream_device` (a BlockMatcher, EXACT mode, its own scene detection), or -- with `warp`, a
    WgpuFrameInterpolator -- `flow.estimate_device_stream` (a FlowEstimator; None: zero flow) and `warp.retime_device`, with `scene`
    (a SceneDetector or None) the detector over all pairs and nus_scene_apply_cuts_retime_device behind it; one download.
    `select` (with `flow` and `warp`): both flows of every pair, `flow.estimate_both_device_stream`, and the select warp,
    `warp.retime_select_device`; scene detection behind it as before.
    The device buffers are torch tensors, so -- as for every device-resident use of the package -- a process imports torch before
    the first call that loads the library (the handles' constructors included)."""
    import torch

    from . import transfer

    if select and (flow is None or warp is None):
        raise ValueError("select needs a flow estimator and a warp (flow=..., warp=...)")
    frames = list(frames)
    n, fb = len(frames), int(w) * int(h) * 4
    num, den = retime_ratio(fps_in, fps_out)
    n_out = retime_count(n, fps_in, fps_out)
    if any(len(memoryview(f).cast("B")) != fb for f in frames):
        raise ValueError(f"every frame must hold {fb} bytes ({w}x{h} RGBA8)")
    dev = f"cuda:{int(device)}"
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream().cuda_stream

        def scratch(nbytes):  # 16-byte aligned device bytes (kept alive by the tensor)
            t = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)
            return t, (t.data_ptr() + 15) & ~15

        d_in = torch.empty((n, fb), dtype=torch.uint8, device=dev)
        for k, f in enumerate(frames):
            transfer.upload(d_in[k].data_ptr(), f, s)
        d_out = torch.empty((n_out, fb), dtype=torch.uint8, device=dev)
        if matcher is not None:
            ws_bytes = matcher.stream_workspace_size(w, h, n)
            ws, d_ws = scratch(ws_bytes)
            matcher.retime_stream_device(d_in.data_ptr(), fb, n, w, h, num, den, d_ws, ws_bytes, d_out.data_ptr(), stream=s)
        else:
            flows = None
            if select:
                flows = torch.empty((2, max(n - 1, 1), h, w, 2), dtype=torch.float32, device=dev)
                flow.estimate_both_device_stream(d_in.data_ptr(), n, w, h, flows[0].data_ptr(), flows[1].data_ptr(), s)
                warp.retime_select_device(d_in.data_ptr(), fb, n, flows[0].data_ptr(), flows[1].data_ptr(), w, h, num, den,
                                          d_out.data_ptr(), 0, s)
            else:
                if flow is not None:
                    flows = torch.empty((n - 1, h, w, 2), dtype=torch.float32, device=dev)
                    flow.estimate_device_stream(d_in.data_ptr(), n, w, h, flows.data_ptr(), s)
                d_flows = flows.data_ptr() if flows is not None else 0
                warp.retime_device(d_in.data_ptr(), fb, n, d_flows, w, h, num, den, d_out.data_ptr(), 0, s)
            if scene is not None:
                ws_bytes = scene.workspace_size(w, h, n - 1)
                ws, d_ws = scratch(ws_bytes)
                cut, d_cut = scratch(n - 1)
                scene.detect_device(d_in.data_ptr(), fb, d_in.data_ptr() + fb, fb, w, h, n - 1, d_ws, ws_bytes, d_cut, stream=s)
                if C.lib().nus_scene_apply_cuts_retime_device(d_in.data_ptr(), fb, n, w, h, C.FORMAT_RGBA8, num, den, d_cut,
                                                              d_out.data_ptr(), 0, s) != C.OK:
                    raise RuntimeError(C.last_error())
        out = transfer.to_numpy(d_out)
    return [out[j].tobytes() for j in range(n_out)]
