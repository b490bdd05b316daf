"""The retained observation's host side (no GPU): td_retain_obs / td_retained_obs are
declared in tdstep.h and bound in gym_TD._lib with the header's types, TD_RETAIN_OBS is
parsed like TD_CONTIG_OBS, and TDEngine checks retain_obs before it touches a device."""
import ctypes
import os
import re
import warnings

import pytest

from gym_TD import _lib
from gym_TD import engine as E

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tdstep.h")


def test_declared_in_the_header_and_bound_with_its_types():
    hdr = open(HEADER).read()
    assert re.search(r"^int td_retain_obs\(td_handle\* h, const void\* obs\);", hdr, re.M)
    assert re.search(r"^const void\* td_retained_obs\(td_handle\* h\);", hdr, re.M)
    assert "#define TD_ABI_VERSION 3" in hdr or _lib.lib.td_abi_version() == 3
    f, g = _lib.lib.td_retain_obs, _lib.lib.td_retained_obs
    assert f.restype is ctypes.c_int and list(f.argtypes) == [ctypes.c_void_p, ctypes.c_void_p]
    assert g.restype is ctypes.c_void_p and list(g.argtypes) == [ctypes.c_void_p]
    assert _lib.lib.td_step_io_size() == 120  # the contract adds nothing to td_step_io


def test_null_handle_is_refused():
    assert _lib.lib.td_retain_obs(None, None) < 0
    assert _lib.lib.td_last_error()
    assert _lib.lib.td_retained_obs(None) is None


@pytest.mark.parametrize("value,want", [(None, True), ("", True), ("1", True), ("true", True), (" On ", True),
                                        ("yes", True), ("0", False), ("false", False), ("No", False), ("off", False)])
def test_env_switch_parsing(value, want):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert E._parse_retain_obs(value) is want


def test_env_switch_unknown_value_warns_and_keeps_the_default():
    with pytest.warns(RuntimeWarning, match="TD_RETAIN_OBS"):
        assert E._parse_retain_obs("maybe") is True


@pytest.mark.parametrize("bad", [None, 1, 0, "yes", "0"])
def test_engine_checks_retain_obs_before_td_create(bad, monkeypatch):
    def no_create(*a, **k):
        raise AssertionError("td_create was reached")
    monkeypatch.setattr(_lib.lib, "td_create", no_create, raising=False)
    with pytest.raises(ValueError, match="retain_obs"):
        E.TDEngine(10, 4, "def", False, 1, device=0, retain_obs=bad)
