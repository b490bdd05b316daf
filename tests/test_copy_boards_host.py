"""td_copy_boards as the header declares it and the ctypes binding binds it, the unchanged ABI,
its refusal of a NULL handle, and its index validation run as a stand-alone host program
under the address and undefined-behaviour sanitizers -- all without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from gym_TD import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tdstep.h")
C_TYPES = {"td_handle*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "float*": ctypes.c_void_p,
           "void*": ctypes.c_void_p, "int": ctypes.c_int}


def _decl(src, name):
    m = re.search(r"^([\w ]+?)\s+%s\(([^)]*)\);" % name, src, re.M)
    assert m, "%s is not declared in tdstep.h" % name
    args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]
    return m.group(1).strip(), args


def test_header_declares_library_exports_binding_binds():
    res, args = _decl(open(HEADER).read(), "td_copy_boards")
    assert (res, args) == ("int", ["td_handle*", "const int32_t*", "const int32_t*", "int", "float*", "void*"])
    fn = _lib.lib.td_copy_boards  # (AttributeError: the library does not export it)
    assert fn.restype == ctypes.c_int
    assert list(fn.argtypes) == [C_TYPES[a] for a in args]
    assert list(fn.argtypes) == [_lib.c_vp, _lib.c_vp, _lib.c_vp, ctypes.c_int, _lib.c_vp, _lib.c_vp]


def test_not_a_diagnostic_hook():
    diag = open(os.path.join(os.path.dirname(HEADER), "td_diag.h")).read()
    assert "td_copy_boards" not in diag and "copy_boards" not in diag


def test_abi_unchanged():
    assert re.search(r"#define TD_ABI_VERSION 3\b", open(HEADER).read())
    assert _lib.ABI_VERSION == 3 and _lib.lib.td_abi_version() == 3
    assert _lib.lib.td_step_io_size() == 120 == ctypes.sizeof(_lib.TdStepIO)
    assert ctypes.sizeof(_lib.TdMaskIO) == 40


def test_header_states_the_contract():
    """The comment above the declaration names what a caller has to know."""
    src = open(HEADER).read()
    at = src.index("int td_copy_boards(")
    doc = src[src.rindex("/*", 0, at):at]
    for word in ("copy.deepcopy", "td_export_state", "td_retained_obs", "random_agent = 0", "random_agent = 1",
                 "named twice in dst", "both src and dst", "n == 0", "epoch"):
        assert word in doc, word


def test_null_handle_is_an_error():
    ids = (ctypes.c_int32 * 2)(0, 1)
    assert _lib.lib.td_copy_boards(None, ids, ids, 1, None, None) < 0
    assert b"td_copy_boards" in _lib.lib.td_last_error()
    assert _lib.lib.td_copy_boards(None, None, None, 0, None, None) < 0


def test_engine_and_vector_env_have_the_methods():
    from gym_TD import envs
    from gym_TD.engine import TDEngine
    assert "deepcopy" in TDEngine.copy_boards.__doc__ and "brought to the host" in TDEngine.copy_boards.__doc__
    assert "until the next step" in TDEngine.copy_boards.__doc__
    assert callable(envs.TDVecEnv.fork)


def test_index_validation_under_sanitizers(tmp_path):
    """scripts/copy_check_host.cpp: duplicates, overlaps, ids out of range and n at both bounds
    through td_copy_check.h's copy_check, the function td_copy_boards calls first, as a
    program of its own built with -fsanitize=address,undefined (any report aborts it)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "copy_check_host")
    src = os.path.join(ROOT, "scripts", "copy_check_host.cpp")
    cc = subprocess.run([cxx] + flags + ["-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.search(r"copy_check: \d+ cases ok", run.stdout), run.stdout
