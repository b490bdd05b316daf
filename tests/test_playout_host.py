"""td_playout and its list forms as the header declares them and the ctypes binding binds them,
the unchanged ABI, td_playout_io_init, the refusals that need no handle, and the whole refusal
table (scripts/playout_check_host.cpp over csrc/td_call_check.h) as a stand-alone program under
the address and undefined-behaviour sanitizers -- all without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from gym_TD import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tdstep.h")
IOP = ctypes.POINTER(_lib.TdPlayoutIO)
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _decl(src, name):
    m = re.search(r"^([\w ]+?[\s*]+)%s\(([^)]*)\);" % name, src, re.M)
    assert m, "%s is not declared" % name
    args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]
    return m.group(1).strip().replace(" *", "*"), args


def test_header_declares_library_exports_binding_binds():
    src = open(HEADER).read()
    want = {
        "td_playout_io_init": ("void", ["td_playout_io*"], None, [IOP]),
        "td_playout": ("int", ["td_handle*", "const td_playout_io*", "void*"], ctypes.c_int, [_lib.c_vp, IOP, _lib.c_vp]),
        "td_playout_boards": ("int", ["td_handle*", "const td_playout_io*", "const int32_t*", "int", "void*"],
                              ctypes.c_int, [_lib.c_vp, IOP, _lib.c_vp, ctypes.c_int, _lib.c_vp]),
        "td_playout_boards_dev": ("int", ["td_handle*", "const td_playout_io*", "const int32_t*", "int",
                                          "const int32_t*", "td_list_status*", "void*"], ctypes.c_int,
                                  [_lib.c_vp, IOP, _lib.c_vp, ctypes.c_int, _lib.c_vp, _lib.c_vp, _lib.c_vp]),
        "td_playout_kernel_name": ("const char*", ["td_handle*"], ctypes.c_char_p, [_lib.c_vp]),
    }
    for name, (res, args, restype, argtypes) in want.items():
        assert _decl(src, name) == (res, args), name
        fn = getattr(_lib.lib, name)  # (AttributeError: the library does not export it)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    assert _lib.lib.td_playout_kernel_name(None) == b""


def test_struct_layout_and_abi_unchanged():
    src = open(HEADER).read()
    assert re.search(r"#define TD_ABI_VERSION 3\b", src)
    assert re.search(r"#define TD_MAX_PLAYOUT_STEPS 4096\b", src) and _lib.MAX_PLAYOUT_STEPS == 4096
    assert _lib.ABI_VERSION == 3 and _lib.lib.td_abi_version() == 3
    assert _lib.lib.td_step_io_size() == 120 == ctypes.sizeof(_lib.TdStepIO)  # additions only
    assert ctypes.sizeof(_lib.TdSampleIO) == 64 and ctypes.sizeof(_lib.TdMaskIO) == 40
    body = re.search(r"typedef struct td_playout_io \{(.*?)\} td_playout_io;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.TdPlayoutIO._fields_], names
    assert ctypes.sizeof(_lib.TdPlayoutIO) == 120
    offs = {f[0]: getattr(_lib.TdPlayoutIO, f[0]).offset for f in _lib.TdPlayoutIO._fields_}
    assert offs == {"size": 0, "abi": 4, "steps": 8, "def_idle": 12, "atk_idle": 16, "reserved": 20, "seed": 24,
                    "ticket": 32, "reward": 40, "done": 48, "steps_run": 56, "win": 64, "allow_next": 72,
                    "cooldowns": 80, "ep_return": 88, "ep_len": 96, "first_def": 104, "first_atk": 112}
    # the field types, as the header writes them
    for name, t in (("steps", "int32_t"), ("reward", r"double\*"), ("done", r"uint8_t\*"), ("steps_run", r"int32_t\*"),
                    ("win", r"int8_t\*"), ("first_def", r"int64_t\*"), ("first_atk", r"int64_t\*")):
        assert re.search(r"\b%s\s+%s;" % (t, name), body), (name, t)


def test_io_init():
    io = _lib.TdPlayoutIO(size=1, abi=9, steps=7, reward=8, seed=5, ticket=6, def_idle=7, atk_idle=8, first_atk=16)
    _lib.lib.td_playout_io_init(ctypes.byref(io))
    assert (io.size, io.abi) == (120, 3)
    assert all(not getattr(io, f[0]) for f in _lib.TdPlayoutIO._fields_[2:])
    _lib.lib.td_playout_io_init(None)  # (a NULL io is left alone)


def _calls():
    lib, ids = _lib.lib, (ctypes.c_int32 * 2)(0, 1)
    return [("td_playout", lambda h, io: lib.td_playout(h, io, None)),
            ("td_playout_boards", lambda h, io: lib.td_playout_boards(h, io, ids, 1, None)),
            ("td_playout_boards_dev", lambda h, io: lib.td_playout_boards_dev(h, io, None, 1, None, None, None))]


def test_io_is_checked_before_the_handle():
    """A NULL io, then the size word, then the abi word, then the handle -- each with the call's
    name; nothing behind the handle is looked at without one."""
    err = _lib.lib.td_last_error
    for name, call in _calls():
        n = name.encode()
        assert call(None, None) < 0 and err() == n + b": NULL io"
        assert call(None, _lib.TdPlayoutIO(size=112)) < 0
        assert err() == n + (b": td_playout_io has size 112 / abi 3, this library expects size 120 / abi 3 "
                             b"(call td_playout_io_init)")
        assert call(None, _lib.TdPlayoutIO(abi=2)) < 0
        assert err().startswith(n + b": td_playout_io has size 120 / abi 2")
        assert call(None, _lib.TdPlayoutIO()) < 0 and err() == n + b": NULL handle"  # (steps = 0 comes behind it)
    assert _lib.lib.td_playout_boards_dev(None, _lib.TdPlayoutIO(), None, -1, None, None, None) < 0
    assert err() == b"td_playout_boards_dev: cap = -1 is negative"
    assert _lib.lib.td_playout_boards_dev(None, _lib.TdPlayoutIO(abi=2), None, -1, None, None, None) < 0
    assert b"abi 2" in err()


def test_refusal_table_as_a_host_program_under_sanitizers(tmp_path):
    """scripts/playout_check_host.cpp: every refusal with its whole message for all three calls,
    and of two faults the one earlier in the order."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + FLAGS + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "playout_check_host")
    cc = subprocess.run([cxx] + FLAGS + ["-o", exe, os.path.join(ROOT, "scripts", "playout_check_host.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"^playout_check: (\d+) cases ok$", run.stdout, re.M)
    assert m and int(m.group(1)) >= 3 * 50, run.stdout
    # the program's constants are the header's
    src = open(os.path.join(ROOT, "scripts", "playout_check_host.cpp")).read()
    assert "kSize = %d" % ctypes.sizeof(_lib.TdPlayoutIO) in src and "kMax = %d" % _lib.MAX_PLAYOUT_STEPS in src


def test_header_states_the_contract():
    src = open(HEADER).read()
    at = src.index("#define TD_MAX_PLAYOUT_STEPS")
    doc = src[src.rindex("/* Random playouts", 0, at):at]
    for word in ("ticket + j", "td_sample_actions", "td_step_boards", "steps_run", "first_def", "TD_FLAG_NO_LAYOUT",
                 "TD_FLAG_BAD_ACTION", "left to right", "refill cadence", "ring guard", "td_kernel_timing",
                 "retained observation", "td_frame_skip()", "multi-action", "random_agent = 0", "td_list_errors",
                 "TD_LIST_TWICE", "at most one staged layout per launch", "lazy-twist", "td_episode_records"):
        assert word in doc, word


def test_engine_and_vector_env_have_the_methods():
    from gym_TD import envs, sampling
    from gym_TD.engine import TDEngine
    assert "td_playout" in TDEngine.playout.__doc__ and "td_playout_boards_dev" in TDEngine.playout_boards_dev.__doc__
    assert "td_playout_kernel_name" in TDEngine.playout_kernel_name.__doc__
    assert envs.TDVecEnv.playout.__doc__ and envs.TDVecEnv.playout_dev.__doc__
    assert "ticket + j" in sampling.reference_playout.__doc__
