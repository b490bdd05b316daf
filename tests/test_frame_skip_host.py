"""Frame skip (td_set_frame_skip / td_frame_skip) as the header declares it and the ctypes
binding binds it, the unchanged ABI, and TDEngine's check of ``frame_skip`` -- all without
a GPU."""
import ctypes
import os
import re

import pytest

from gym_TD import _lib
from gym_TD.engine import TDEngine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tdstep.h")
C_TYPES = {"td_handle*": ctypes.c_void_p, "int": ctypes.c_int}


def _decl(src, name):
    m = re.search(r"^([\w ]+?)\s+%s\(([^)]*)\);" % name, src, re.M)
    assert m, "%s is not declared in tdstep.h" % name
    args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]
    return m.group(1).strip(), args


@pytest.mark.parametrize("name", ["td_set_frame_skip", "td_frame_skip"])
def test_header_declares_and_library_exports(name):
    src = open(HEADER).read()
    res, args = _decl(src, name)
    fn = getattr(_lib.lib, name)  # (AttributeError: the library does not export it)
    assert fn.restype == C_TYPES[res], (name, res)
    assert list(fn.argtypes) == [C_TYPES[a] for a in args], (name, args)


def test_not_a_diagnostic_hook():
    diag = open(os.path.join(os.path.dirname(HEADER), "td_diag.h")).read()
    assert "frame_skip" not in diag


def test_limit_and_abi_unchanged():
    src = open(HEADER).read()
    m = re.search(r"#define TD_MAX_FRAME_SKIP (\d+)\b", src)
    assert m and int(m.group(1)) == 16 == _lib.MAX_FRAME_SKIP
    assert re.search(r"#define TD_ABI_VERSION 3\b", src)
    assert _lib.ABI_VERSION == 3 and _lib.lib.td_abi_version() == 3
    assert _lib.lib.td_step_io_size() == 120 == ctypes.sizeof(_lib.TdStepIO)  # the skip is no field of td_step_io


def test_null_handle_is_an_error():
    assert _lib.lib.td_frame_skip(None) < 0
    assert _lib.lib.td_set_frame_skip(None, 2) < 0
    assert _lib.lib.td_last_error()


@pytest.mark.parametrize("k", [0, 17, 2.5, -1, "4", None, True])
def test_engine_refuses_bad_frame_skip_before_any_device_call(k, monkeypatch):
    def no_create(*a):
        raise AssertionError("td_create was called")
    monkeypatch.setattr(_lib.lib, "td_create", no_create)
    with pytest.raises(ValueError, match="frame_skip"):
        TDEngine(10, 4, "def", False, 1, device=0, frame_skip=k)
