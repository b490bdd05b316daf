"""td_sample_actions and its list forms as the header declares them and the ctypes binding binds
them, the unchanged ABI, td_sample_io_init, and the refusals that need no handle -- all without
a GPU."""
import ctypes
import os
import re

from gym_TD import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tdstep.h")
IOP = ctypes.POINTER(_lib.TdSampleIO)


def _decl(src, name):
    m = re.search(r"^([\w ]+?[\s*]+)%s\(([^)]*)\);" % name, src, re.M)
    assert m, "%s is not declared" % name
    args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]
    return m.group(1).strip().replace(" *", "*"), args


def test_header_declares_library_exports_binding_binds():
    src = open(HEADER).read()
    want = {
        "td_sample_io_init": ("void", ["td_sample_io*"], None, [IOP]),
        "td_sample_actions": ("int", ["td_handle*", "const td_sample_io*", "void*"], ctypes.c_int, [_lib.c_vp, IOP, _lib.c_vp]),
        "td_sample_actions_boards": ("int", ["td_handle*", "const td_sample_io*", "const int32_t*", "int", "void*"],
                                     ctypes.c_int, [_lib.c_vp, IOP, _lib.c_vp, ctypes.c_int, _lib.c_vp]),
        "td_sample_actions_boards_dev": ("int", ["td_handle*", "const td_sample_io*", "const int32_t*", "int",
                                                 "const int32_t*", "td_list_status*", "void*"], ctypes.c_int,
                                         [_lib.c_vp, IOP, _lib.c_vp, ctypes.c_int, _lib.c_vp, _lib.c_vp, _lib.c_vp]),
        "td_sample_actions_kernel_name": ("const char*", ["td_handle*"], ctypes.c_char_p, [_lib.c_vp]),
    }
    for name, (res, args, restype, argtypes) in want.items():
        assert _decl(src, name) == (res, args), name
        fn = getattr(_lib.lib, name)  # (AttributeError: the library does not export it)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    assert _lib.lib.td_sample_actions_kernel_name(None) == b""


def test_struct_layout_and_abi_unchanged():
    src = open(HEADER).read()
    assert re.search(r"#define TD_ABI_VERSION 3\b", src)
    assert _lib.ABI_VERSION == 3 and _lib.lib.td_abi_version() == 3
    assert _lib.lib.td_step_io_size() == 120 == ctypes.sizeof(_lib.TdStepIO)  # additions only
    body = re.search(r"typedef struct td_sample_io \{(.*?)\} td_sample_io;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.TdSampleIO._fields_], names
    assert ctypes.sizeof(_lib.TdSampleIO) == 64
    offs = {f[0]: getattr(_lib.TdSampleIO, f[0]).offset for f in _lib.TdSampleIO._fields_}
    assert offs == {"size": 0, "abi": 4, "def_act": 8, "atk_act": 16, "def_count": 24, "atk_count": 32, "seed": 40,
                    "ticket": 48, "def_idle": 56, "atk_idle": 60}


def test_io_init():
    io = _lib.TdSampleIO(size=1, abi=9, def_act=8, seed=5, ticket=6, def_idle=7, atk_idle=8)
    _lib.lib.td_sample_io_init(ctypes.byref(io))
    assert (io.size, io.abi) == (64, 3)
    assert all(not getattr(io, f[0]) for f in _lib.TdSampleIO._fields_[2:])
    _lib.lib.td_sample_io_init(None)  # (a NULL io is left alone)


def _calls():
    lib, ids = _lib.lib, (ctypes.c_int32 * 2)(0, 1)
    return [("td_sample_actions", lambda h, io: lib.td_sample_actions(h, io, None)),
            ("td_sample_actions_boards", lambda h, io: lib.td_sample_actions_boards(h, io, ids, 1, None)),
            ("td_sample_actions_boards_dev", lambda h, io: lib.td_sample_actions_boards_dev(h, io, None, 1, None, None, None))]


def test_io_is_checked_before_the_handle():
    """A NULL io, then the size word, then the abi word, then the handle -- each with the call's name."""
    err = _lib.lib.td_last_error
    for name, call in _calls():
        n = name.encode()
        assert call(None, None) < 0 and err() == n + b": NULL io"
        assert call(None, _lib.TdSampleIO(size=56)) < 0
        assert err() == n + b": td_sample_io has size 56 / abi 3, this library expects size 64 / abi 3 (call td_sample_io_init)"
        assert call(None, _lib.TdSampleIO(abi=2)) < 0
        assert err().startswith(n + b": td_sample_io has size 64 / abi 2")
        assert call(None, _lib.TdSampleIO()) < 0 and err() == n + b": NULL handle"
    # the device-list form refuses a negative cap with the io words alone
    assert _lib.lib.td_sample_actions_boards_dev(None, _lib.TdSampleIO(), None, -1, None, None, None) < 0
    assert err() == b"td_sample_actions_boards_dev: cap = -1 is negative"
    assert _lib.lib.td_sample_actions_boards_dev(None, _lib.TdSampleIO(abi=2), None, -1, None, None, None) < 0
    assert b"abi 2" in err()


def test_header_states_the_contract():
    src = open(HEADER).read()
    at = src.index("typedef struct td_sample_io")
    doc = src[src.rindex("/* One uniformly drawn", 0, at):at]
    for word in ("0x9E3779B97F4A7C15", "4 b + j", "def_idle", "n / 2^32", "no rejection loop", "board id, not the list position",
                 "td_list_errors", "td_frame_skip() > 1", "td_kernel_timing", "refill cadence", "no action output wanted",
                 "FailCode 0", "ascending"):
        assert word in doc, word


def test_engine_and_vector_env_have_the_methods():
    from gym_TD import envs
    from gym_TD.engine import TDEngine
    for name in ("sample_actions", "sample_actions_boards", "sample_actions_boards_dev"):
        assert name.replace("sample", "td_sample") in getattr(TDEngine, name).__doc__
        assert getattr(envs.TDVecEnv, name).__doc__
    assert "ticket" in TDEngine.sample_actions.__doc__ and "sample_seed" in TDEngine.__doc__
