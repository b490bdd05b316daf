"""The observation-format calls (td_set_obs_format / td_obs_format / td_obs_bytes) as the
header declares them and the ctypes binding binds them, and the dtype check of TDEngine --
all without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from gym_TD import _lib
from gym_TD import vector
from gym_TD.engine import OBS_FORMATS, TDEngine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tdstep.h")
C_TYPES = {"td_handle*": ctypes.c_void_p, "int": ctypes.c_int, "size_t": ctypes.c_size_t}


def _decl(src, name):
    m = re.search(r"^([\w ]+?)\s+%s\(([^)]*)\);" % name, src, re.M)
    assert m, "%s is not declared in tdstep.h" % name
    args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]
    return m.group(1).strip(), args


@pytest.mark.parametrize("name", ["td_set_obs_format", "td_obs_format", "td_obs_bytes"])
def test_header_and_binding_agree(name):
    src = open(HEADER).read()
    res, args = _decl(src, name)
    fn = getattr(_lib.lib, name)
    assert fn.restype == C_TYPES[res], (name, res)
    assert list(fn.argtypes) == [C_TYPES[a] for a in args], (name, args)


def test_format_enum_and_abi_unchanged():
    src = open(HEADER).read()
    assert re.search(r"enum td_obs_format \{ TD_OBS_F32 = 0, TD_OBS_F16 = 1 \};", src)
    assert (_lib.OBS_F32, _lib.OBS_F16) == (0, 1)
    assert OBS_FORMATS == {torch.float32: 0, torch.float16: 1}
    assert re.search(r"#define TD_ABI_VERSION 3\b", src)
    assert _lib.ABI_VERSION == 3 and _lib.lib.td_abi_version() == 3
    assert _lib.lib.td_step_io_size() == 120 == ctypes.sizeof(_lib.TdStepIO)  # the format is no field of td_step_io


@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16, torch.int16, None])
def test_engine_refuses_other_dtypes_before_td_create(dtype, monkeypatch):
    def no_create(*a):
        raise AssertionError("td_create was called")
    monkeypatch.setattr(_lib.lib, "td_create", no_create)
    with pytest.raises(ValueError, match="obs_dtype"):
        TDEngine(10, 4, "def", False, 1, device=0, obs_dtype=dtype)


def test_vector_env_refuses_other_dtypes():
    with pytest.raises(ValueError, match="obs_dtype"):
        vector.VectorEnv("TD-def-small-v0", 2, obs_dtype="float64")
