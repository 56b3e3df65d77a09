"""nus_flow_fill_workspace (TEST HOOK) without a GPU: the export, the header's prototype and the sys crate in step, the refusal
unless the process has NUS_TEST_HOOKS=1 (read per call), the refusal of a value that is no byte, and the no-op -- NUS_OK before
any HIP call -- on a null handle and on a handle that has reserved nothing.  The stream rule the GPU tests hold the handle to
(tests/test_gpu_flow_workspace.py) is in the header and in INTEGRATION.md."""
import os

import pytest

from conftest import ROOT

NAME = "nus_flow_fill_workspace"


@pytest.fixture(scope="module")
def lib(nsc):
    return nsc._capi.lib()


@pytest.fixture
def flow(lib):
    h = lib.nus_flow_create()
    assert h
    yield h
    lib.nus_flow_destroy(h)


def test_export_header_and_sys_crate(nsc, lib):
    assert hasattr(lib, NAME)
    assert (NAME, nsc._capi._i, [nsc._capi._vp, nsc._capi._i, nsc._capi._vp]) in [tuple(s) for s in nsc._capi.SIGNATURES]
    hdr = open(os.path.join(ROOT, "include", "nuscaler_hip.h")).read()
    proto = "int nus_flow_fill_workspace(nus_flow *h, int byte_value, void *stream);"
    assert proto in hdr
    comment = hdr[:hdr.index(proto)].rsplit("/*", 1)[1]  # the comment in front of the prototype says what it is
    assert comment.lstrip().startswith("TEST HOOK") and "NUS_TEST_HOOKS=1" in comment
    assert "#define NUS_ABI_VERSION 1\n" in hdr and lib.nus_abi_version() == 1
    sys_rs = open(os.path.join(ROOT, "rust", "nu_scaler_hip-sys", "src", "lib.rs")).read()
    assert "pub fn nus_flow_fill_workspace(h: *mut nus_flow, byte_value: c_int, stream: *mut c_void) -> c_int;" in sys_rs
    # the stream rule, where an integrator reads it
    assert "THE STREAM RULE" in hdr and hdr.index("THE STREAM RULE") < hdr.index("int nus_flow_estimate_device(")
    assert "stream rule" in open(os.path.join(ROOT, "INTEGRATION.md")).read().lower()


def test_refused_without_the_variable(nsc, lib, flow, monkeypatch):
    inv = nsc._capi.ERR_INVALID_ARGUMENT
    for value in (None, "0", "", "true", "11", " 1"):  # only "1" asks for the hooks
        if value is None:
            monkeypatch.delenv("NUS_TEST_HOOKS", raising=False)
        else:
            monkeypatch.setenv("NUS_TEST_HOOKS", value)
        assert lib.nus_flow_fill_workspace(flow, 0, None) == inv, value
        msg = lib.nus_flow_last_error(flow).decode()
        assert msg.startswith("nus_flow_fill_workspace:"), msg
        assert nsc._capi.last_error() == msg
    monkeypatch.setenv("NUS_TEST_HOOKS", "1")  # read per call: the same handle, the next call
    assert lib.nus_flow_fill_workspace(flow, 0, None) == nsc._capi.OK
    monkeypatch.delenv("NUS_TEST_HOOKS")
    assert lib.nus_flow_fill_workspace(flow, 0, None) == inv


def test_refuses_what_is_no_byte(nsc, lib, flow, monkeypatch):
    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    for bad in (256, -1, 257, 1 << 20, -(1 << 31)):
        assert lib.nus_flow_fill_workspace(flow, bad, None) == nsc._capi.ERR_INVALID_ARGUMENT, bad
        assert lib.nus_flow_last_error(flow).decode().startswith("nus_flow_fill_workspace:")
    assert lib.nus_flow_workspace_bytes(flow) == 0


def test_no_op_on_a_handle_that_holds_nothing(nsc, lib, flow, monkeypatch):
    """No device is needed (this test runs without one): a fresh handle has reserved nothing, so no HIP call is made."""
    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    for byte in (0x00, 0xFF, 0x7F, 0x3E, 255):
        assert lib.nus_flow_fill_workspace(flow, byte, None) == nsc._capi.OK
        assert lib.nus_flow_fill_workspace(None, byte, None) == nsc._capi.OK  # a null handle holds nothing either
    assert lib.nus_flow_workspace_bytes(flow) == 0
    assert lib.nus_flow_mode(flow) == 0 and lib.nus_flow_warps(flow) == 0 and lib.nus_flow_median_size(flow) == 0  # nothing moved


def test_python_wrapper(nsc, monkeypatch):
    from nu_scaler_amd.flow import FlowEstimator

    f = FlowEstimator()
    monkeypatch.delenv("NUS_TEST_HOOKS", raising=False)
    with pytest.raises(RuntimeError, match="^nus_flow_fill_workspace:"):
        f._fill_workspace(0)
    monkeypatch.setenv("NUS_TEST_HOOKS", "1")
    f._fill_workspace(0x3E)
    f._fill_workspace(0xFF, stream=0)
    with pytest.raises(RuntimeError, match="^nus_flow_fill_workspace:"):
        f._fill_workspace(256)
    assert f.workspace_bytes == 0
    assert "_fill_workspace" not in [n for n in dir(FlowEstimator) if not n.startswith("_")]  # private: a hook, not an API
