"""td_probe and its list forms as the header declares them and the ctypes binding binds them, the
unchanged ABI, td_probe_io_init, the struct's layout in C and in ctypes, and the refusals that
need no handle in their order -- all without a GPU."""
import ctypes
import re

from gym_TD import _lib
from test_playout_host import HEADER, _decl

IOP = ctypes.POINTER(_lib.TdProbeIO)
SIZE = 88


def test_header_declares_library_exports_binding_binds():
    src = open(HEADER).read()
    want = {
        "td_probe_io_init": ("void", ["td_probe_io*"], None, [IOP]),
        "td_probe": ("int", ["td_handle*", "const td_probe_io*", "void*"], ctypes.c_int, [_lib.c_vp, IOP, _lib.c_vp]),
        "td_probe_boards": ("int", ["td_handle*", "const td_probe_io*", "const int32_t*", "int", "void*"],
                            ctypes.c_int, [_lib.c_vp, IOP, _lib.c_vp, ctypes.c_int, _lib.c_vp]),
        "td_probe_boards_dev": ("int", ["td_handle*", "const td_probe_io*", "const int32_t*", "int",
                                        "const int32_t*", "td_list_status*", "void*"], ctypes.c_int,
                                [_lib.c_vp, IOP, _lib.c_vp, ctypes.c_int, _lib.c_vp, _lib.c_vp, _lib.c_vp]),
        "td_probe_kernel_name": ("const char*", ["td_handle*"], ctypes.c_char_p, [_lib.c_vp]),
    }
    for name, (res, args, restype, argtypes) in want.items():
        assert _decl(src, name) == (res, args), name
        fn = getattr(_lib.lib, name)  # (AttributeError: the library does not export it)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    assert _lib.lib.td_probe_kernel_name(None) == b""


def test_struct_layout_and_abi_unchanged():
    src = open(HEADER).read()
    assert re.search(r"#define TD_ABI_VERSION 3\b", src)
    assert re.search(r"#define TD_MAX_PROBE_REPS 256\b", src) and _lib.MAX_PROBE_REPS == 256
    assert _lib.ABI_VERSION == 3 and _lib.lib.td_abi_version() == 3
    # additions only: the structs that were there keep their sizes
    assert _lib.lib.td_step_io_size() == 120 == ctypes.sizeof(_lib.TdStepIO)
    assert ctypes.sizeof(_lib.TdSampleIO) == 64 and ctypes.sizeof(_lib.TdMaskIO) == 40
    assert ctypes.sizeof(_lib.TdPlayoutIO) == 120
    body = re.search(r"typedef struct td_probe_io \{(.*?)\} td_probe_io;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.TdProbeIO._fields_], names
    assert names == ["size", "abi", "steps", "reps", "def_idle", "atk_idle", "seed", "ticket", "reward", "done",
                     "steps_run", "win", "first_def", "first_atk"]
    offs = {f[0]: getattr(_lib.TdProbeIO, f[0]).offset for f in _lib.TdProbeIO._fields_}
    assert offs == {"size": 0, "abi": 4, "steps": 8, "reps": 12, "def_idle": 16, "atk_idle": 20, "seed": 24,
                    "ticket": 32, "reward": 40, "done": 48, "steps_run": 56, "win": 64, "first_def": 72,
                    "first_atk": 80}
    for name, t in (("steps", "int32_t"), ("reps", "int32_t"), ("reward", r"double\*"), ("done", r"uint8_t\*"),
                    ("steps_run", r"int32_t\*"), ("win", r"int8_t\*"), ("first_def", r"int64_t\*"),
                    ("first_atk", r"int64_t\*")):
        assert re.search(r"\b%s\s+%s;" % (t, name), body), (name, t)


def test_struct_size_agrees_between_c_and_ctypes():
    """td_probe_io_init writes sizeof(td_probe_io) as the C compiler sees it into the size word."""
    io = _lib.TdProbeIO(size=0)
    _lib.lib.td_probe_io_init(ctypes.byref(io))
    assert io.size == ctypes.sizeof(_lib.TdProbeIO) == SIZE


def test_io_init():
    io = _lib.TdProbeIO(size=1, abi=9, steps=7, reps=5, reward=8, seed=5, ticket=6, def_idle=7, atk_idle=8, first_atk=16)
    _lib.lib.td_probe_io_init(ctypes.byref(io))
    assert (io.size, io.abi) == (SIZE, 3)
    assert all(not getattr(io, f[0]) for f in _lib.TdProbeIO._fields_[2:])
    _lib.lib.td_probe_io_init(None)  # (a NULL io is left alone)


def _calls():
    lib, ids = _lib.lib, (ctypes.c_int32 * 2)(0, 1)
    return [("td_probe", lambda h, io: lib.td_probe(h, io, None)),
            ("td_probe_boards", lambda h, io: lib.td_probe_boards(h, io, ids, 1, None)),
            ("td_probe_boards_dev", lambda h, io: lib.td_probe_boards_dev(h, io, None, 1, None, None, None))]


def test_io_is_checked_before_the_handle():
    """A NULL io, then the size word, then the abi word, then the handle -- each with the call's
    name; nothing behind the handle (steps, reps, the outputs) is looked at without one."""
    err = _lib.lib.td_last_error
    for name, call in _calls():
        n = name.encode()
        assert call(None, None) < 0 and err() == n + b": NULL io"
        assert call(None, _lib.TdProbeIO(size=120)) < 0  # (a td_playout_io is not taken for one)
        assert err() == n + (b": td_probe_io has size 120 / abi 3, this library expects size 88 / abi 3 "
                             b"(call td_probe_io_init)")
        assert call(None, _lib.TdProbeIO(abi=2)) < 0
        assert err().startswith(n + b": td_probe_io has size 88 / abi 2")
        # steps = 0, reps = 0 and the missing outputs all come behind the handle
        assert call(None, _lib.TdProbeIO()) < 0 and err() == n + b": NULL handle"
        assert call(None, _lib.TdProbeIO(steps=3, reps=300)) < 0 and err() == n + b": NULL handle"
    assert _lib.lib.td_probe_boards_dev(None, _lib.TdProbeIO(), None, -1, None, None, None) < 0
    assert err() == b"td_probe_boards_dev: cap = -1 is negative"
    assert _lib.lib.td_probe_boards_dev(None, _lib.TdProbeIO(abi=2), None, -1, None, None, None) < 0
    assert b"abi 2" in err()


def test_header_states_the_contract():
    src = open(HEADER).read()
    at = src.index("#define TD_MAX_PROBE_REPS")
    doc = src[src.rindex("/* Probes", 0, at):at]
    for word in ("ticket + r * steps", "td_playout_boards", "steps * reps", "same position", "sampled side only",
                 "TD_FLAG_NO_LAYOUT", "lazy-twist", "hot record", "td_episode_records", "layout rings", "refill cadence",
                 "ring guard", "td_retain_obs", "td_kernel_timing", "td_list_errors", "[B][reps]", "td_frame_skip()",
                 "multi-action", "random_agent = 0", "named twice", "TD_MAX_PROBE_REPS"):
        assert word in doc, word


def test_engine_and_vector_env_have_the_methods():
    from gym_TD import envs, sampling
    from gym_TD.engine import TDEngine
    assert "td_probe" in TDEngine.probe.__doc__ and "td_probe_boards_dev" in TDEngine.probe_boards_dev.__doc__
    assert "td_probe_kernel_name" in TDEngine.probe_kernel_name.__doc__
    assert envs.TDVecEnv.probe.__doc__ and envs.TDVecEnv.probe_dev.__doc__
    assert "ticket + r * steps" in sampling.reference_probe.__doc__
