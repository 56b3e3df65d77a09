"""The launch arithmetic of the Horn-Schunck Jacobi kernels (launch_hs_iterate, nus_k_flow.hip), restated without HIP, and CASES:
the one table tests/test_gpu_flow_steps.py runs and tests/test_flow_steps_census.py holds against the instantiations the
compiler emits.

Three kernel families take their steps per launch K as a template argument; an instantiation is written here as a tuple
    ("tiled", T, K, NT)          k_hs_tiled<T, K, NT>            T x T cells per tile, NT threads
    ("stream", K, LUM, UPS)      k_hs_stream<K, LUM, UPS>        LUM: derivatives from the luminance planes, UPS: and the coarser
                                                                 level's flow upsampled as it is loaded
    ("fast", K, UPS, RING)       k_hs_stream_fast<K, UPS, RING>  RING: the queues in rings (the product's form), else shifting
A level's `iterations` steps are ceil(iterations / maxk) launches of evenly many steps each."""
from collections import namedtuple

WAVE = 64
STREAM_MAX_K = 5       # kHsStreamMaxK
FAST_MAX_K = 5         # kHsFastMaxK
FAST_MAX_K_LONG = 8    # kHsFastMaxKLong: a level of at least FAST_LONG_STEPS steps
FAST_LONG_STEPS = 30
TILED_MAX_K = 8        # kHsTiledMaxK: Small and Mid tiles; every tile class is instantiated up to it
BIG_MAX_K = 5          # kHsBigMaxK
TILE_CLASSES = {"small": (16, 1024), "mid": (32, 1024), "big": (32, 256)}  # class: (T, NT)
STREAM_MIN_ROWS = 64   # kHsStreamMinRows
MAX_CHUNK_PAIRS = 150  # kStreamMaxChunkPairs: a stream of more pairs goes through the levels in chunks


def cdiv(a, b):
    return (a + b - 1) // b


def split(iterations, maxk):
    """The steps of each launch of a level: ceil(iterations / maxk) launches, each time k = ceil(left / launches left)."""
    launches = cdiv(iterations, maxk)
    out = []
    while iterations > 0:
        k = cdiv(iterations, launches)
        out.append(k)
        iterations -= k
        launches -= 1
    return out


def tile_class(w, h, n):
    """The LDS-tile kernel's class from the number of 32 x 32 tiles the whole batch has."""
    tiles32 = cdiv(w, 32) * cdiv(h, 32) * n
    return "big" if tiles32 >= 1024 else ("mid" if tiles32 >= 256 else "small")


def maxk(family, iterations=0, cls=None):
    if family == "stream":
        return STREAM_MAX_K
    if family == "fast":
        return FAST_MAX_K_LONG if iterations >= FAST_LONG_STEPS else FAST_MAX_K
    if family == "tiled":
        return BIG_MAX_K if cls == "big" else TILED_MAX_K
    raise ValueError(family)


def strips(w, k):
    """Strips of a streamed launch of k steps: a wave's 64 lanes carry k halo columns on each side."""
    return cdiv(w, WAVE - 2 * k)


def stream_row_blocks(w, h, n, k):
    """(row blocks, rows per block) of a forced streamed launch (hs_stream_shape with force: never back to the tiles)."""
    simds = 1024
    columns = strips(w, k) * n
    max_blocks = max(h // STREAM_MIN_ROWS, 1)
    best, shape = None, (1, h)
    for rb in range(1, max_blocks + 1):
        rows = cdiv(h, rb)
        if cdiv(h, rows) != rb:
            continue
        waves = columns * rb
        if waves < 3 * simds and rb != max_blocks:
            continue
        cost = cdiv(waves, simds) * (rows + 3 * k)
        if best is None or cost < best:
            best, shape = cost, (rb, rows)
    return shape


def level_sizes(w, h, levels):
    """[(w, h)] of the pyramid, finest first: next = (cur + 1) / 2, nothing below 1 x 1."""
    out = []
    for _ in range(levels):
        out.append((w, h))
        if (w, h) == (1, 1):
            break
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


def reachable(family, cls=None, upto=2000):
    """{(K, first launch of its level or not)} over every step count 0 .. upto."""
    out = set()
    for n in range(upto + 1):
        for i, k in enumerate(split(n, maxk(family, n, cls))):
            out.add((k, i == 0))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# entry: "horn_schunck" (the primitive: one level, one pair, `coarse` steps on coefficient planes, start "zero" or "random"),
#        "stream" (estimate_device_stream; with the streamed kernels also estimate_device on frames 1 and 2),
#        "fast" (estimate_device_stream in FAST, ring form and shifting form), "handoff" (interpolate_device_stream in FAST, f16 flows)
# tiled: what set_tiled takes (2: LDS tiles, 3: the streamed kernels); frames: RGBA8 frames of the stream (pairs = frames - 1)
# target: the instantiation the row is there for; also: further ones its launches reach that no row of their own covers
Case = namedtuple("Case", "id group target also entry tiled mode levels coarse refine w h frames content")


def _case(id, group, target, entry, tiled, levels, coarse, refine, w, h, frames=2, mode="exact", also=(), content="noise"):
    return Case(id, group, target, tuple(also), entry, tiled, mode, levels, coarse, refine, w, h, frames, content)


def _strip_widths(k):
    s = WAVE - 2 * k
    return (s, s + 1, 2 * s + 1)  # one strip, the first column of a second one, the first column of a third


def _build_cases():
    rows = []
    # a. streamed, coefficient form
    for k in range(1, 6):
        for w in _strip_widths(k):
            for h in (33, 129):  # 129: two row blocks
                rows.append(_case(f"a-stream-coef-k{k}-{w}x{h}", "a", ("stream", k, False, False), "horn_schunck", 3, 1, k, 0, w, h))
    rows.append(_case("a-stream-coef-n7-113x129", "a", ("stream", 4, False, False), "horn_schunck", 3, 1, 7, 0, 113, 129))  # 4, 3
    rows.append(_case("a-stream-coef-n9-109x129", "a", ("stream", 5, False, False), "horn_schunck", 3, 1, 9, 0, 109, 129))  # 5, 4
    # b. LDS tiles, Small
    for k in range(1, 9):
        for w, h in ((16, 16), (17, 17), (47, 33)):  # one tile, one cell past it both ways, ragged
            rows.append(_case(f"b-small-k{k}-{w}x{h}", "b", ("tiled", 16, k, 1024), "horn_schunck", 2, 1, k, 0, w, h))
    rows.append(_case("b-small-n13-47x33", "b", ("tiled", 16, 7, 1024), "horn_schunck", 2, 1, 13, 0, 47, 33))  # 7, 6
    # c. LDS tiles, Mid and Big: 130 x 70 frames are 5 x 3 tiles of 32, 18 pairs 270 of them, 69 pairs 1035
    for k in range(1, 9):
        rows.append(_case(f"c-mid-k{k}", "c", ("tiled", 32, k, 1024), "stream", 2, 1, k, 0, 130, 70, frames=19))
    for k in range(1, 6):
        rows.append(_case(f"c-big-k{k}", "c", ("tiled", 32, k, 256), "stream", 2, 1, k, 0, 130, 70, frames=70))
    rows.append(_case("c-big-n6", "c", ("tiled", 32, 3, 256), "stream", 2, 1, 6, 0, 130, 70, frames=70))  # 3, 3
    # level 0: 69 pairs, Big, 2 steps; level 1: 65 x 35, 3 x 2 x 69 = 414 tiles, Mid, 3 steps
    rows.append(_case("c-big-k2-over-mid-k3", "c", ("tiled", 32, 2, 256), "stream", 2, 2, 3, 2, 130, 70, frames=70,
                      also=[("tiled", 32, 3, 1024)]))
    # d. streamed, plane forms; the pair entry takes the coefficient form
    for k in range(1, 6):
        for w in _strip_widths(k):
            rows.append(_case(f"d-stream-planes-k{k}-{w}x70", "d", ("stream", k, True, False), "stream", 3, 1, k, 0, w, 70, frames=4,
                              also=[("stream", k, False, False)]))
            rows.append(_case(f"d-stream-ups-k{k}-{w}x70", "d", ("stream", k, True, True), "stream", 3, 2, 3, k, w, 70, frames=4,
                              also=[("stream", 3, True, False), ("stream", k, False, False), ("stream", 3, False, False)]))
    # e. FAST: both ring forms of every row
    def fast(k, ups):
        return ("fast", k, ups, True)

    def both(*insts):  # the shifting form of every instantiation named
        return [("fast", k, ups, False) for (_, k, ups, _) in insts]

    for n, k, more in ((1, 1, ()), (2, 2, ()), (3, 3, ()), (4, 4, ()), (5, 5, ()), (30, 8, (fast(7, False),)), (33, 6, (fast(7, False),))):
        w = 2 * (WAVE - 2 * k) + 1
        for content in (("smooth", "noise") if n <= 5 else ("smooth",)):
            rows.append(_case(f"e-fast-n{n}-{w}x70-{content}", "e", fast(k, False), "fast", 3, 1, n, 0, w, 70, frames=4, mode="fast",
                              also=list(more) + both(fast(k, False), *more), content=content))
    for n, k, more in ((1, 1, ()), (2, 2, ()), (3, 3, ()), (4, 4, ()), (5, 5, ()), (35, 7, (fast(7, False),)), (40, 8, (fast(8, False),))):
        w = 2 * (WAVE - 2 * k) + 1
        for content in (("smooth", "noise") if n <= 5 else ("smooth",)):
            rows.append(_case(f"e-fast-ups-n{n}-{w}x70-{content}", "e", fast(k, True), "fast", 3, 2, 5, n, w, 70, frames=4, mode="fast",
                              also=[fast(5, False)] + list(more) + both(fast(k, True), fast(5, False), *more), content=content))
    # two row blocks, 8 / 7 / 6 halo rows each side
    rows.append(_case("e-fast-n33-129x129-smooth", "e", fast(6, False), "fast", 3, 1, 33, 0, 129, 129, frames=4, mode="fast",
                      also=[fast(7, False)] + both(fast(6, False), fast(7, False)), content="smooth"))
    rows.append(_case("e-fast-ups-n40-129x129-smooth", "e", fast(8, True), "fast", 3, 2, 5, 40, 129, 129, frames=4, mode="fast",
                      also=[fast(8, False)] + both(fast(8, True), fast(8, False)), content="smooth"))
    # f. the Rg16Float store of the level's last launch
    for n in (1, 2, 3, 4):
        w = 2 * (WAVE - 2 * n) + 1
        rows.append(_case(f"f-half-ups-k{n}-{w}x70", "f", fast(n, True), "handoff", 3, 2, 5, n, w, 70, frames=4, mode="fast",
                          content="smooth"))
    rows.append(_case("f-half-k6-105x70", "f", fast(6, False), "handoff", 3, 1, 33, 0, 105, 70, frames=4, mode="fast", content="smooth"))
    return tuple(rows)


CASES = _build_cases()


def group(name):
    return [c for c in CASES if c.group == name]


# Instantiations the library holds and launch_hs_iterate cannot reach, each with its reason (kept, not removed: taking them out
# changes the build)
UNREACHABLE = {}
for _k in (6, 7, 8):
    UNREACHABLE[("tiled", 32, _k, 256)] = "the Big tile class is launched with maxk = 5 (kHsBigMaxK)"
for _ring in (True, False):
    UNREACHABLE[("fast", 6, True, _ring)] = ("a first launch of 6 steps needs a level of >= 30 steps (maxk = 8) in L launches with "
                                            "8 (L - 1) < steps <= 6 L, so L < 4 and steps <= 24")


def launched(case):
    """Every instantiation the case launches, by the restated schedule: the coarsest level `coarse` steps from zero flow, each finer
    level `refine` steps from the level below (warps, median: off)."""
    pairs = case.frames - 1
    assert pairs <= MAX_CHUNK_PAIRS, "one chunk: the tile class is that of the whole stream"
    out = set()

    def steps(w, h, n, iterations, lum, ups, fast_forms=()):
        if case.tiled == 2:
            cls = tile_class(w, h, n)
            t, nt = TILE_CLASSES[cls]
            out.update(("tiled", t, k, nt) for k in split(iterations, maxk("tiled", iterations, cls)))
        elif fast_forms:
            for i, k in enumerate(split(iterations, maxk("fast", iterations))):
                out.update(("fast", k, ups and i == 0, ring) for ring in fast_forms)
        else:
            for i, k in enumerate(split(iterations, maxk("stream"))):
                out.add(("stream", k, lum, lum and ups and i == 0))

    sizes = level_sizes(case.w, case.h, case.levels)
    if case.entry == "horn_schunck":
        steps(case.w, case.h, 1, case.coarse, False, False)
        return out
    runs = [(sizes[-1], case.coarse, False)] + [(sz, case.refine, True) for sz in reversed(sizes[:-1])]
    for (w, h), iterations, ups in runs:
        if case.entry == "stream":
            steps(w, h, pairs, iterations, True, ups)
            if case.tiled == 3:  # and estimate_device on one pair: coefficient planes, the flow upsampled by the level's setup kernel
                steps(w, h, 1, iterations, False, False)
        elif case.entry == "fast":
            steps(w, h, pairs, iterations, True, ups, fast_forms=(True, False))
        elif case.entry == "handoff":
            steps(w, h, pairs, iterations, True, ups, fast_forms=(True,))
        else:
            raise ValueError(case.entry)
    return out


def parse_label(label):
    """The instantiation a mangled kernel name stands for, or None: name and template arguments only."""
    import re

    m = re.search(r"\d+(k_hs_tiled|k_hs_stream_fast|k_hs_stream)I((?:L[ib]\d+E)+)E", label)
    if not m:
        return None
    args = [int(v) if t == "i" else bool(int(v)) for t, v in re.findall(r"L([ib])(\d+)E", m.group(2))]
    return ({"k_hs_tiled": "tiled", "k_hs_stream": "stream", "k_hs_stream_fast": "fast"}[m.group(1)],) + tuple(args)


def parse_demangled(name):
    """The same from a demangled name, as a kernel trace prints it: `... k_hs_stream<5, true, false>(...)`."""
    import re

    m = re.search(r"\b(k_hs_tiled|k_hs_stream_fast|k_hs_stream)<([^>]*)>", name)
    if not m:
        return None
    args = [a.strip() == "true" if a.strip() in ("true", "false") else int(a) for a in m.group(2).split(",")]
    return ({"k_hs_tiled": "tiled", "k_hs_stream": "stream", "k_hs_stream_fast": "fast"}[m.group(1)],) + tuple(args)


def show(inst):
    fam = {"tiled": "k_hs_tiled", "stream": "k_hs_stream", "fast": "k_hs_stream_fast"}[inst[0]]
    return fam + "<" + ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in inst[1:]) + ">"
