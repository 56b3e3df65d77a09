"""The rate-conversion schedule of include/nuscaler_hip.h ("Frame-rate conversion by a rational ratio") restated in Python ints
and np.float32, for the tests of the retime entry points.  Not the package's mirror (nu_scaler_amd/retime.py): written from the
header's statement alone."""
from math import gcd

import numpy as np

MAX_TERM = 4096
MAX_RATIO = 8


def reduce(num, den):
    g = gcd(num, den)
    return num // g, den // g


def count(n_frames, num, den):
    num, den = reduce(num, den)
    return ((n_frames - 1) * num) // den + 1


def schedule(n_frames, num, den):
    """[(k_j, r_j, t_j)] with t_j an np.float32."""
    num, den = reduce(num, den)
    out = []
    for j in range(count(n_frames, num, den)):
        k, r = (j * den) // num, (j * den) % num
        out.append((k, r, np.float32(r) / np.float32(num)))  # one f32 division of two exactly held integers
    return out


def schedule_array(n_frames, num, den, first=0, count=None):
    """Entries first .. first + count - 1 (default: to the end) of the same table as as_array lays it out, (count, 4) uint32,
    vectorised for streams of a million frames: j den in uint64 (below 2^45 for every stream the library takes), its quotient and
    remainder by num, and ONE np.float32 division of the remainder (below 4096: exact in f32) by num."""
    num, den = reduce(num, den)
    n_out = ((n_frames - 1) * num) // den + 1
    cnt = n_out - first if count is None else count
    assert 0 <= first and 0 <= cnt and first + cnt <= n_out, (first, cnt, n_out)
    at = np.arange(first, first + cnt, dtype=np.uint64) * np.uint64(den)
    k, r = at // np.uint64(num), at % np.uint64(num)
    a = np.zeros((cnt, 4), np.uint32)
    a[:, 0], a[:, 1] = k, r
    a[:, 2] = (r.astype(np.float32) / np.float32(num)).view(np.uint32)
    return a


def times_of(table):
    """The t column of a schedule_array / as_array table as np.float32."""
    return np.ascontiguousarray(table[:, 2]).view(np.float32)


def first_output(pair, num, den):
    """Index of the first output at or behind frame `pair`: ceil(pair num / den), in Python ints."""
    num, den = reduce(num, den)
    return -((-pair * num) // den)


def as_array(entries):
    """The table as the library lays it out: n x {u32 pair, u32 rem, f32 t, u32 0} viewed as (n, 4) uint32."""
    a = np.zeros((len(entries), 4), np.uint32)
    for j, (k, r, t) in enumerate(entries):
        a[j, 0], a[j, 1] = k, r
        a[j, 2] = np.float32(t).view(np.uint32)
    return a
