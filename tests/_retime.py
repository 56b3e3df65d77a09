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


def as_array(entries):
    """The table as the library lays it out: n x {u32 pair, u32 rem, f32 t, u32 0} viewed as (n, 4) uint32."""
    a = np.zeros((len(entries), 4), np.uint32)
    for j, (k, r, t) in enumerate(entries):
        a[j, 0], a[j, 1] = k, r
        a[j, 2] = np.float32(t).view(np.uint32)
    return a
