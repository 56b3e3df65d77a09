"""nus_bm_set_bidirectional without a GPU: the export, the header's prototype and default, the argument checks (before any HIP
call, the text begins with the entry point's name), both workspace sizes with the mode on, off and off again, the Python
wrappers' arguments and the flag of the Python CLI.  The native CLI takes the same arguments."""
import os
import subprocess

import pytest

from conftest import ROOT

DA, DB, DWS, DVEC = (0x7F0000000000 + k * 0x10000000 for k in range(4))  # fake device addresses, never touched
SHAPES = [(1, 1, 1), (7, 5, 3), (33, 17, 2), (200, 72, 4), (1920, 1080, 1), (1920, 1080, 16)]  # w, h, pairs


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


@pytest.fixture
def bm(lib):
    h = lib.nus_bm_create()
    assert h
    yield h
    lib.nus_bm_destroy(h)


def _err(lib, h):
    return lib.nus_bm_last_error(h).decode()


def test_export_header_and_default(nsc, lib):
    assert hasattr(lib, "nus_bm_set_bidirectional")
    assert any(s[0] == "nus_bm_set_bidirectional" for s in nsc._capi.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    assert "int nus_bm_set_bidirectional(nus_blockmatch *h, int enabled, uint32_t tolerance);" in hdr
    assert "#define NUS_BM_BIDIR_DEFAULT_TOLERANCE 2\n" in hdr
    assert nsc._capi.BM_BIDIR_DEFAULT_TOLERANCE == 2
    assert "#define NUS_ABI_VERSION 1\n" in hdr
    sys_rs = open(os.path.join(ROOT, "rust", "nu_scaler_hip-sys", "src", "lib.rs")).read()
    assert "pub fn nus_bm_set_bidirectional(h: *mut nus_blockmatch, enabled: c_int, tolerance: u32) -> c_int;" in sys_rs


def test_argument_checks(nsc, lib, bm):
    ok, inv = nsc._capi.OK, nsc._capi.ERR_INVALID_ARGUMENT
    assert lib.nus_bm_set_bidirectional(None, 1, 2) == inv and nsc._capi.last_error() == "null handle"
    for enabled in (0, 1):
        for tol in (0, 2, 96):
            assert lib.nus_bm_set_bidirectional(bm, enabled, tol) == ok
    for enabled, tol in ((2, 2), (-1, 2)):
        assert lib.nus_bm_set_bidirectional(bm, enabled, tol) == inv
        assert _err(lib, bm).startswith("nus_bm_set_bidirectional:"), _err(lib, bm)
    for tol in (97, 1 << 31, (1 << 32) - 1):
        assert lib.nus_bm_set_bidirectional(bm, 1, tol) == inv
        msg = _err(lib, bm)
        assert msg.startswith("nus_bm_set_bidirectional:") and "tolerance" in msg, msg
        assert nsc._capi.last_error() == msg


def test_both_workspaces_grow_only_while_the_mode_is_on(nsc, lib, bm):
    ok = nsc._capi.OK
    for q, bs in ((0, 8), (1, 16), (2, 32)):
        assert lib.nus_bm_set_quality(bm, q) == ok
        for w, h, n in SHAPES:
            off = (lib.nus_bm_workspace_size(bm, w, h, n), lib.nus_bm_stream_workspace_size(bm, w, h, n + 1))
            assert off[0] > 0 and off[1] > 0
            assert lib.nus_bm_set_bidirectional(bm, 1, 2) == ok
            on = (lib.nus_bm_workspace_size(bm, w, h, n), lib.nus_bm_stream_workspace_size(bm, w, h, n + 1))
            # per block: the backward vector and SAD, the forward SAD, the chosen vector (4 bytes each) and a state byte
            blocks = n * -(-w // bs) * -(-h // bs)
            assert on[0] >= off[0] + 17 * blocks and on[1] >= off[1] + 17 * blocks, (bs, w, h, n, off, on)
            assert abs((on[1] - off[1]) - (on[0] - off[0])) < 16  # the stream's workspace grows by the search's part, padded to 16
            assert lib.nus_bm_set_bidirectional(bm, 0, 2) == ok
            again = (lib.nus_bm_workspace_size(bm, w, h, n), lib.nus_bm_stream_workspace_size(bm, w, h, n + 1))
            assert again == off, (bs, w, h, n)


def test_a_workspace_of_the_old_size_is_refused_with_the_mode_on(nsc, lib, bm):
    w, h = 64, 32
    fb = w * h * 4
    off = lib.nus_bm_workspace_size(bm, w, h, 1)
    assert lib.nus_bm_set_bidirectional(bm, 1, 2) == nsc._capi.OK
    on = lib.nus_bm_workspace_size(bm, w, h, 1)
    st = lib.nus_bm_estimate_device(bm, DA, fb, DB, fb, w, h, 1, DWS, off, DVEC, None, None, None, 0, None)
    assert st == nsc._capi.ERR_INVALID_ARGUMENT
    msg = _err(lib, bm)
    assert msg.startswith("nus_bm_estimate_device:") and "nus_bm_workspace_size" in msg and str(on) in msg, msg


def test_python_wrappers(nsc):
    m = nsc.BlockMatcher("medium")
    assert m.bidirectional is False and m.tolerance == 2
    off = (m.workspace_size(200, 72, 2), m.stream_workspace_size(200, 72, 3))
    m.set_bidirectional(True)
    assert m.bidirectional is True and m.tolerance == 2
    assert m.workspace_size(200, 72, 2) > off[0] and m.stream_workspace_size(200, 72, 3) > off[1]
    m.set_bidirectional(True, 4)
    assert m.tolerance == 4
    with pytest.raises(ValueError, match="nus_bm_set_bidirectional"):
        m.set_bidirectional(True, 97)
    assert m.tolerance == 4  # a rejected call changes nothing
    m.set_bidirectional(False)
    assert (m.workspace_size(200, 72, 2), m.stream_workspace_size(200, 72, 3)) == off
    on = nsc.BlockMatcher("high", bidirectional=True, tolerance=0)
    assert on.bidirectional and on.tolerance == 0 and on.workspace_size(200, 72) > nsc.BlockMatcher("high").workspace_size(200, 72)
    it = nsc.PyFrameInterpolator("block_matching", "low", bidirectional=True)
    assert it.name == "BlockMatching" and it._bm.bidirectional
    assert not nsc.PyFrameInterpolator("block_matching")._bm.bidirectional
    with pytest.raises(ValueError, match="bidirectional"):
        nsc.PyFrameInterpolator("optical_flow", bidirectional=True)


def test_python_cli_flag(nsc, capsys):
    from nu_scaler_amd import cli

    p = cli.build_parser()
    base = ["interpolate", "a.png", "b.png", "out.png", "--method", "block_matching"]
    a = p.parse_args(base)
    assert a.bidirectional is False and a.bidir_tolerance is None
    a = p.parse_args(base + ["--bidirectional"])
    assert a.bidirectional is True and a.bidir_tolerance is None
    a = p.parse_args(base + ["--bidirectional", "--bidir-tolerance", "4"])
    assert a.bidirectional is True and a.bidir_tolerance == 4
    for argv, text in ((base + ["--bidirectional", "--bidir-tolerance", "97"], "--bidir-tolerance must be from 0 to 96"),
                       (base + ["--bidir-tolerance", "4"], "--bidir-tolerance needs --bidirectional"),
                       (["interpolate", "a.png", "b.png", "out.png", "--bidirectional"], "--bidirectional needs --method")):
        with pytest.raises(SystemExit) as e:  # usage errors: status 2 before anything is read
            cli.main(argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err


@pytest.mark.parametrize("extra,text", [
    (["--method", "block_matching", "--bidirectional", "--bidir-tolerance", "97"], "--bidir-tolerance must be from 0 to 96"),
    (["--method", "block_matching", "--bidirectional", "--bidir-tolerance", "x"], "--bidir-tolerance must be from 0 to 96"),
    (["--method", "block_matching", "--bidir-tolerance", "4"], "--bidir-tolerance needs --bidirectional"),
    (["--bidirectional"], "--bidirectional needs --method block_matching"),
    (["--flow", "--bidirectional"], "--bidirectional needs --method block_matching"),
])
def test_native_cli_usage_errors(nsc, tmp_path, extra, text):
    cli = os.path.join(ROOT, "nu_scaler_amd", "bin", "nu_scaler_cli")
    assert os.path.exists(cli), "the native CLI is built with the library"
    out = str(tmp_path / "mid.png")
    r = subprocess.run([cli, "interpolate", str(tmp_path / "a.png"), str(tmp_path / "b.png"), out] + extra, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and text in r.stderr, (r.returncode, r.stderr)  # before anything is read: the frames do not exist
    assert not os.path.exists(out)
    assert "--bidirectional" in r.stderr  # the usage text names the flag
