"""Which steps-per-launch instantiations of the Horn-Schunck Jacobi kernels can run, and that each of them has a GPU case: the
launch arithmetic restated in tests/_hs_steps.py, enumerated, and held against the kernel labels hipcc emits for nus_k_flow.hip.
No GPU.  Raising a steps-per-launch limit, adding a kernel form or dropping a row of CASES fails here."""
import os
import re
import subprocess

import pytest

import _hs_steps as hs
from conftest import ROOT

CSRC = os.path.join(ROOT, "nu_scaler_amd", "csrc")


def test_the_split_is_even_and_complete():
    assert hs.split(0, 5) == []
    assert hs.split(7, 5) == [4, 3] and hs.split(9, 5) == [5, 4] and hs.split(13, 8) == [7, 6] and hs.split(6, 5) == [3, 3]
    assert hs.split(30, 8) == [8, 8, 7, 7] and hs.split(33, 8) == [7, 7, 7, 6, 6] and hs.split(35, 8) == [7] * 5 and hs.split(40, 8) == [8] * 5
    assert hs.split(50, 8) == [8, 7, 7, 7, 7, 7, 7] and hs.split(50, 5) == [5] * 10 and hs.split(10, 5) == [5, 5]
    for maxk in (5, 8):
        for n in range(1, 400):
            s = hs.split(n, maxk)
            assert sum(s) == n and len(s) == hs.cdiv(n, maxk) and max(s) - min(s) <= 1 and s == sorted(s, reverse=True), (n, maxk, s)
    assert hs.maxk("fast", 29) == 5 and hs.maxk("fast", 30) == 8 and hs.maxk("tiled", 50, "big") == 5 and hs.maxk("tiled", 50, "mid") == 8


def test_the_constants_are_the_kernel_file_s():
    src = open(os.path.join(CSRC, "nus_k_flow.hip")).read()

    def const(name):
        return int(re.search(r"\b" + name + r" = (\d+)", src).group(1))

    assert (const("kHsStreamMaxK"), const("kHsFastMaxK"), const("kHsFastMaxKLong"), const("kHsTiledMaxK"), const("kHsBigMaxK")) == \
        (hs.STREAM_MAX_K, hs.FAST_MAX_K, hs.FAST_MAX_K_LONG, hs.TILED_MAX_K, hs.BIG_MAX_K)
    assert (const("kHsBigT"), const("kHsBigThreads")) == hs.TILE_CLASSES["big"]
    assert (const("kHsMidT"), const("kHsMidThreads")) == hs.TILE_CLASSES["mid"]
    assert (const("kHsSmallT"), const("kHsSmallThreads")) == hs.TILE_CLASSES["small"]
    assert const("kHsStreamMinRows") == hs.STREAM_MIN_ROWS
    assert f"L.iterations >= {hs.FAST_LONG_STEPS} ? kHsFastMaxKLong : kHsFastMaxK" in src
    assert "tiles32 >= 1024 ? 2 : (tiles32 >= 256 ? 1 : 0)" in src
    hdr = open(os.path.join(CSRC, "nus_flow.hpp")).read()
    assert int(re.search(r"kStreamMaxChunkPairs = (\d+)", hdr).group(1)) == hs.MAX_CHUNK_PAIRS


def test_reachable_steps_per_launch():
    def ks(reached, first):
        return {k for k, f in reached if f == first}

    # a level's first launch is its longest; a later one exists only beyond maxk steps, which even out above maxk / 2
    assert ks(hs.reachable("stream"), True) == {1, 2, 3, 4, 5} and ks(hs.reachable("stream"), False) == {3, 4, 5}
    for cls in ("small", "mid"):
        assert ks(hs.reachable("tiled", cls), True) == {1, 2, 3, 4, 5, 6, 7, 8} and ks(hs.reachable("tiled", cls), False) == {4, 5, 6, 7, 8}
    big = hs.reachable("tiled", "big")  # 6, 7, 8 instantiated, never launched
    assert ks(big, True) == {1, 2, 3, 4, 5} and ks(big, False) == {3, 4, 5}
    fast = hs.reachable("fast")
    assert ks(fast, True) == {1, 2, 3, 4, 5, 7, 8}  # a level never starts with a launch of 6 steps
    assert ks(fast, False) == {3, 4, 5, 6, 7, 8}
    # the step counts behind the two FAST forms the rest of the suite never launches
    assert [n for n in range(50) if 6 in hs.split(n, hs.maxk("fast", n))] == [33, 34, 41]
    assert [n for n in range(50) if hs.split(n, hs.maxk("fast", n))[:1] == [7]] == [33, 34, 35, 41, 42, 49]


def _reachable_instantiations():
    out = set()
    for cls, (t, nt) in hs.TILE_CLASSES.items():
        out |= {("tiled", t, k, nt) for k, _ in hs.reachable("tiled", cls)}
    for k, first in hs.reachable("stream"):
        out |= {("stream", k, False, False), ("stream", k, True, False)}
        if first:
            out.add(("stream", k, True, True))  # only a level's first launch takes the coarser level's flow
    for k, first in hs.reachable("fast"):
        for ring in (True, False):
            out.add(("fast", k, False, ring))
            if first:
                out.add(("fast", k, True, ring))
    return out


def _covered(cases):
    out = set()
    for c in cases:
        out.add(c.target)
        out.update(c.also)
    return out


def test_every_case_launches_what_it_claims():
    ids = [c.id for c in hs.CASES]
    assert len(set(ids)) == len(ids)
    for c in hs.CASES:
        got = hs.launched(c)
        assert c.target in got, (c.id, hs.show(c.target), sorted(map(hs.show, got)))
        assert set(c.also) <= got, (c.id, sorted(map(hs.show, set(c.also) - got)))
        assert max(c.w, c.h) <= 130, c.id
        # the K the row names is in the split of its step counts, and its tile class follows from size and pair count
        k = c.target[2] if c.target[0] == "tiled" else c.target[1]
        fam = c.target[0]
        sizes = hs.level_sizes(c.w, c.h, c.levels)
        n = 1 if c.entry == "horn_schunck" else c.frames - 1
        splits = []
        for l, (w, h) in enumerate(sizes):
            steps = c.coarse if l == len(sizes) - 1 else c.refine
            cls = hs.tile_class(w, h, n) if fam == "tiled" else None
            if fam != "tiled" or hs.TILE_CLASSES[cls] == (c.target[1], c.target[3]):
                splits += hs.split(steps, hs.maxk(fam, steps, cls))
        assert k in splits, (c.id, k, splits)
    by_id = {c.id: c for c in hs.CASES}
    assert hs.tile_class(130, 70, 18) == "mid" and hs.tile_class(130, 70, 69) == "big" and hs.tile_class(65, 35, 69) == "mid"
    assert hs.tile_class(47, 33, 1) == "small"
    assert by_id["c-mid-k8"].frames == 19 and by_id["c-big-k5"].frames == 70
    # group a: one strip, the first column of a second and of a third one; 129 rows are two row blocks, 33 rows one
    for c in hs.group("a") + hs.group("d"):
        k = max(hs.split(c.coarse if c.group == "a" else (c.refine or c.coarse), hs.STREAM_MAX_K))
        assert hs.strips(c.w, k) in (1, 2, 3) and (hs.strips(c.w - 1, k) < hs.strips(c.w, k) or hs.strips(c.w + 1, k) > hs.strips(c.w, k)), c.id
        assert hs.stream_row_blocks(c.w, c.h, 1, k)[0] == (2 if c.h == 129 else 1), c.id
    assert {hs.strips(c.w, c.coarse) for c in hs.group("a") if c.coarse <= 5} == {1, 2, 3}
    for c in hs.group("f"):  # the launch that stores the halves is the level's last
        steps = c.refine if c.levels > 1 else c.coarse
        assert hs.split(steps, hs.maxk("fast", steps))[-1] == c.target[1], c.id


def test_every_reachable_instantiation_has_a_case_and_nothing_else_is_claimed():
    reachable = _reachable_instantiations()
    covered = _covered(hs.CASES)
    assert covered <= reachable, sorted(map(hs.show, covered - reachable))
    assert reachable <= covered, sorted(map(hs.show, reachable - covered))
    assert not (set(hs.UNREACHABLE) & reachable)
    assert set(hs.UNREACHABLE) == {("tiled", 32, k, 256) for k in (6, 7, 8)} | {("fast", 6, True, ring) for ring in (True, False)}
    assert all(isinstance(r, str) and r for r in hs.UNREACHABLE.values())


@pytest.fixture(scope="module")
def flow_labels(tmp_path_factory):
    """The kernel labels of nus_k_flow.hip as the library's build compiles it (device only, to assembly)."""
    out = tmp_path_factory.mktemp("asm") / "nus_k_flow.s"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
           "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(out),
           os.path.join(CSRC, "nus_k_flow.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr
    labels = []
    with open(out) as f:
        for line in f:  # names only: a label line, never instruction text
            m = re.match(r"(_Z\w*k_hs_(?:tiled|stream)\w*):", line)
            if m:
                labels.append(m.group(1))
    return labels


def test_built_with_the_makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-O3 -std=c++17 -fPIC -ffp-contract=off" in mk
    assert "nus_k_flow.hip" in mk.split("KERNELS", 1)[1].split("\n", 1)[0]


def census(labels, cases, unreachable):
    """(instantiations with neither a case nor a reason, unreachable entries that are not in the library)."""
    built = {hs.parse_label(l) for l in labels}
    assert None not in built and len(built) == len(labels), "a k_hs_* label the census cannot read"
    return built - _covered(cases) - set(unreachable), set(unreachable) - built


def test_symbol_census(flow_labels):
    assert len(flow_labels) == 3 * 8 + 5 * 3 + 8 * 4  # tile classes x K, K x stream forms, K x FAST forms
    orphans, stale = census(flow_labels, hs.CASES, hs.UNREACHABLE)
    assert not orphans, "instantiations without a GPU case: " + ", ".join(sorted(map(hs.show, orphans)))
    assert not stale, "UNREACHABLE names what the library does not hold: " + ", ".join(sorted(map(hs.show, stale)))
    built = {hs.parse_label(l) for l in flow_labels}
    assert _covered(hs.CASES) <= built  # a case that names a kernel nobody compiled


def test_the_census_notices_a_missing_row_and_a_missing_reason(flow_labels):
    """The rows of every instantiation (one row where it has only one), and every UNREACHABLE entry, taken out in turn: the census
    reports what lost its case."""
    sole = 0
    for inst in _covered(hs.CASES):
        rest = tuple(c for c in hs.CASES if inst != c.target and inst not in c.also)
        sole += len(rest) == len(hs.CASES) - 1
        assert inst in census(flow_labels, rest, hs.UNREACHABLE)[0], hs.show(inst)
    assert sole >= 10  # (the Mid and Big tile classes: one row per K)
    for inst in hs.UNREACHABLE:
        fewer = {k: v for k, v in hs.UNREACHABLE.items() if k != inst}
        assert census(flow_labels, hs.CASES, fewer)[0] == {inst}
    # what raising kHsStreamMaxK to 6 would add to the library
    more = flow_labels + [l.replace("ILi5E", "ILi6E") for l in flow_labels if "11k_hs_streamILi5E" in l]
    assert census(more, hs.CASES, hs.UNREACHABLE)[0] == {("stream", 6, lum, ups) for lum, ups in ((False, False), (True, False), (True, True))}


def test_demangled_names_parse_to_the_same_instantiations():
    assert hs.parse_demangled("void nus::(anonymous namespace)::k_hs_stream_fast<7, true, false>(float const*, unsigned long)") == \
        ("fast", 7, True, False)
    assert hs.parse_demangled("nus::(anonymous namespace)::k_hs_tiled<32, 5, 256>(float const*)") == ("tiled", 32, 5, 256)
    assert hs.parse_demangled("k_hs_stream<5, true, true>") == ("stream", 5, True, True)
    assert hs.parse_demangled("k_hs_prepare<float>") is None
    assert hs.parse_label("_ZN3nus12_GLOBAL__N_111k_hs_streamILi5ELb1ELb0EEEvPKfmf") == ("stream", 5, True, False)
    for inst in _reachable_instantiations():
        assert hs.parse_demangled(hs.show(inst)) == inst
