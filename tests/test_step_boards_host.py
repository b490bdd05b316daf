"""td_step_boards as the header declares it and the ctypes binding binds it, the unchanged ABI,
its refusals that need no device, and its board-list validation run as a stand-alone host
program under the address and undefined-behaviour sanitizers -- all without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from gym_TD import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tdstep.h")
DIAG = os.path.join(ROOT, "include", "td_diag.h")


def _decl(src, name):
    m = re.search(r"^([\w ]+?[\s*]+)%s\(([^)]*)\);" % name, src, re.M)
    assert m, "%s is not declared" % name
    args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]
    return m.group(1).strip().replace(" *", "*"), args


def test_header_declares_library_exports_binding_binds():
    res, args = _decl(open(HEADER).read(), "td_step_boards")
    assert (res, args) == ("int", ["td_handle*", "const td_step_io*", "const int32_t*", "int", "void*"])
    fn = _lib.lib.td_step_boards  # (AttributeError: the library does not export it)
    assert fn.restype == ctypes.c_int
    assert list(fn.argtypes) == [_lib.c_vp, ctypes.POINTER(_lib.TdStepIO), _lib.c_vp, ctypes.c_int, _lib.c_vp]


def test_the_name_function_stands_beside_td_step_kernel_name():
    """In the drop-in header, next to td_step_kernel_name (td_diag.h keeps its four test hooks)."""
    src = open(HEADER).read()
    res, args = _decl(src, "td_step_boards_kernel_name")
    assert (res, args) == ("const char*", ["td_handle*"])
    assert src.index("td_step_kernel_name(td_handle* h);") < src.index("td_step_boards_kernel_name(td_handle* h);")
    assert "td_step_boards_kernel_name" not in open(DIAG).read()
    fn = _lib.lib.td_step_boards_kernel_name
    assert fn.restype == ctypes.c_char_p and list(fn.argtypes) == [_lib.c_vp]
    assert fn(None) == b""


def test_abi_unchanged():
    assert re.search(r"#define TD_ABI_VERSION 3\b", open(HEADER).read())
    assert _lib.ABI_VERSION == 3 and _lib.lib.td_abi_version() == 3
    assert _lib.lib.td_step_io_size() == 120 == ctypes.sizeof(_lib.TdStepIO)


def test_header_states_the_contract():
    """The comment above the declaration names what a caller has to know."""
    src = open(HEADER).read()
    at = src.index("int td_step_boards(")
    doc = src[src.rindex("/*", 0, at):at]
    for word in ("td_copy_boards", "child.step", "indexed by board id", "no byte of an", "td_episode_stats",
                 "n == 0", "td_retained_obs", "TD_FLAG_NO_LAYOUT", "named twice", "td_frame_skip() > 1",
                 "random_agent = 0 with auto-reset", "ring guard", "td_kernel_timing"):
        assert word in doc, word


def test_io_is_checked_before_the_handle():
    """As td_step: a NULL io, then the size / abi words, then the handle -- each with the call's name."""
    ids = (ctypes.c_int32 * 2)(0, 1)
    lib = _lib.lib
    assert lib.td_step_boards(None, None, ids, 1, None) < 0 and b"td_step_boards: NULL io" in lib.td_last_error()
    io = _lib.TdStepIO()
    io.abi = 2
    assert lib.td_step_boards(None, io, ids, 1, None) < 0
    assert lib.td_last_error().startswith(b"td_step_boards: td_step_io has size 120 / abi 2")
    io = _lib.TdStepIO(size=112)
    assert lib.td_step_boards(None, io, ids, 1, None) < 0 and b"size 112" in lib.td_last_error()
    assert lib.td_step_boards(None, _lib.TdStepIO(), None, 0, None) < 0
    assert lib.td_last_error() == b"td_step_boards: NULL handle"
    # td_step's own messages keep td_step's name
    assert lib.td_step(None, None, None) < 0 and lib.td_last_error() == b"td_step: NULL io"
    assert lib.td_step(None, _lib.TdStepIO(), None) < 0 and lib.td_last_error() == b"td_step: NULL handle"


def test_engine_and_vector_env_have_the_methods():
    from gym_TD import envs
    from gym_TD.engine import TDEngine
    doc = TDEngine.step_boards.__doc__
    for word in ("td_step_boards", "copy_boards", "full-batch", "none twice", "host_io", "frame_skip"):
        assert word in doc, word
    assert "action_mask=True" in envs.TDVecEnv.step_boards.__doc__


def test_list_validation_under_sanitizers(tmp_path):
    """scripts/ids_check_host.cpp: n = 0 and n = B, a duplicate at both ends of the list, ids -1
    and B through td_ids_check.h's ids_check, the function td_step_boards calls before it
    enqueues anything, as a program of its own built with -fsanitize=address,undefined (any
    report aborts it); the scratch is all zero after accepted and refused lists alike."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "ids_check_host")
    src = os.path.join(ROOT, "scripts", "ids_check_host.cpp")
    cc = subprocess.run([cxx] + flags + ["-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.search(r"ids_check: \d+ cases ok", run.stdout), run.stdout
