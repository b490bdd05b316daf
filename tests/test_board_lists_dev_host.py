"""td_step_boards_dev / td_copy_boards_dev / td_list_errors as the header declares them and the
ctypes binding binds them, the unchanged ABI, their refusals that need no device, and the
retained-observation ledger's device-list cases run as a stand-alone host program under the
address and undefined-behaviour sanitizers -- all without a GPU."""
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
    src = open(HEADER).read()
    vp, ci, io = _lib.c_vp, ctypes.c_int, ctypes.POINTER(_lib.TdStepIO)
    want = {
        "td_step_boards_dev": (["td_handle*", "const td_step_io*", "const int32_t*", "int", "const int32_t*",
                                "td_list_status*", "void*"], [vp, io, vp, ci, vp, vp, vp]),
        "td_copy_boards_dev": (["td_handle*", "const int32_t*", "const int32_t*", "int", "const int32_t*", "float*",
                                "td_list_status*", "void*"], [vp, vp, vp, ci, vp, vp, vp, vp]),
        "td_list_errors": (["td_handle*", "td_list_status*", "int"], [vp, ctypes.POINTER(_lib.TdListStatus), ci]),
    }
    for name, (cargs, pyargs) in want.items():
        assert _decl(src, name) == ("int", cargs), name
        fn = getattr(_lib.lib, name)  # (AttributeError: the library does not export it)
        assert fn.restype == ctypes.c_int and list(fn.argtypes) == pyargs, name


def test_the_name_function_stands_beside_td_step_boards_kernel_name():
    src = open(HEADER).read()
    assert _decl(src, "td_step_boards_dev_kernel_name") == ("const char*", ["td_handle*"])
    assert src.index("td_step_boards_kernel_name(td_handle* h);") < src.index("td_step_boards_dev_kernel_name(td_handle* h);")
    assert "td_step_boards_dev_kernel_name" not in open(DIAG).read()
    fn = _lib.lib.td_step_boards_dev_kernel_name
    assert fn.restype == ctypes.c_char_p and list(fn.argtypes) == [_lib.c_vp]
    assert fn(None) == b""


def test_abi_unchanged_and_the_status_record_is_16_bytes():
    src = open(HEADER).read()
    assert re.search(r"#define TD_ABI_VERSION 3\b", src)
    assert _lib.ABI_VERSION == 3 and _lib.lib.td_abi_version() == 3
    assert _lib.lib.td_step_io_size() == 120 == ctypes.sizeof(_lib.TdStepIO)
    assert re.search(r"typedef struct td_list_status \{ int32_t code, call, entry, board; \} td_list_status;", src)
    assert ctypes.sizeof(_lib.TdListStatus) == 16
    assert [n for n, _ in _lib.TdListStatus._fields_] == ["code", "call", "entry", "board"]
    assert re.search(r"enum td_list_code \{ TD_LIST_OK = 0, TD_LIST_BAD_COUNT = 1, TD_LIST_RANGE = 2, TD_LIST_TWICE = 3, "
                     r"TD_LIST_OVERLAP = 4 \};", src)
    assert (_lib.LIST_OK, _lib.LIST_BAD_COUNT, _lib.LIST_RANGE, _lib.LIST_TWICE, _lib.LIST_OVERLAP) == (0, 1, 2, 3, 4)


def _doc(src, decl):
    """The comment above a declaration, its line breaks and their " * " taken out."""
    at = src.index(decl)
    return re.sub(r"\s*\n \*\s*", " ", src[src.rindex("/*", 0, at):at])


def test_header_states_the_contract():
    """The comments above the declarations name what a caller has to know."""
    src = open(HEADER).read()
    doc = _doc(src, "enum td_list_code {")
    for word in ("td_step_boards", "td_copy_boards", "byte for byte", "count_dev", "[0, cap]", "never read",
                 "must be final, in stream order", "stay unchanged until the call's kernels have run",
                 "Refused on the host", "Refused on the device", "TD_LIST_BAD_COUNT", "TD_LIST_RANGE", "TD_LIST_TWICE",
                 "TD_LIST_OVERLAP", "cap == 0", "td_frame_skip() > 1", "random_agent = 0 with auto-reset",
                 "td_retained_obs", "EVERY board's row is known", "never makes the handle claim more", "ring guard",
                 "td_kernel_timing", "td_list_errors", "0-based serial", "entry is -1"):
        assert word in doc, word
    doc = _doc(src, "int td_copy_boards_dev(")
    for word in ("src_dev[i]", "count_dev", "lifetime", "status_dev", "TD_LIST_TWICE in dst", "TD_LIST_OVERLAP",
                 "NULL handle", "td_retained_obs", "NULL included", "td_kernel_timing", "td_step_boards_dev"):
        assert word in doc, word
    doc = _doc(src, "int td_list_errors(")
    for word in ("since the last clear", "first of them", "synchronous", "td_guard_timeouts"):
        assert word in doc, word


def test_host_refusals_that_need_no_device():
    """As td_step: a NULL io, then the size / abi words, then the handle -- each with the call's
    own name; cap < 0 needs no handle either."""
    ids = (ctypes.c_int32 * 2)(0, 1)
    lib = _lib.lib
    step = lib.td_step_boards_dev
    assert step(None, None, ids, 1, None, None, None) < 0 and lib.td_last_error() == b"td_step_boards_dev: NULL io"
    io = _lib.TdStepIO()
    io.abi = 2
    assert step(None, io, ids, 1, None, None, None) < 0
    assert lib.td_last_error().startswith(b"td_step_boards_dev: td_step_io has size 120 / abi 2")
    io = _lib.TdStepIO(size=112)
    assert step(None, io, ids, 1, None, None, None) < 0
    assert lib.td_last_error().startswith(b"td_step_boards_dev: td_step_io has size 112")
    # the words come before cap, cap before the handle
    assert step(None, io, ids, -1, None, None, None) < 0 and b"size 112" in lib.td_last_error()
    assert step(None, _lib.TdStepIO(), None, 0, None, None, None) < 0
    assert lib.td_last_error() == b"td_step_boards_dev: NULL handle"
    assert step(None, _lib.TdStepIO(), ids, -1, None, None, None) < 0
    assert lib.td_last_error() == b"td_step_boards_dev: cap = -1 is negative"
    copy = lib.td_copy_boards_dev
    assert copy(None, ids, ids, 1, None, None, None, None) < 0 and lib.td_last_error() == b"td_copy_boards_dev: NULL handle"
    assert copy(None, ids, ids, -3, None, None, None, None) < 0
    assert lib.td_last_error() == b"td_copy_boards_dev: cap = -3 is negative"
    assert lib.td_list_errors(None, None, 0) < 0 and lib.td_last_error() == b"td_list_errors: NULL handle"
    # the host-list calls keep their own names
    assert lib.td_step_boards(None, None, ids, 1, None) < 0 and lib.td_last_error() == b"td_step_boards: NULL io"
    assert lib.td_copy_boards(None, ids, ids, 1, None, None) < 0 and lib.td_last_error() == b"td_copy_boards: NULL handle"


def test_engine_and_vector_env_have_the_methods():
    from gym_TD import envs
    from gym_TD.engine import TDEngine
    doc = TDEngine.step_boards_dev.__doc__
    for word in ("td_step_boards_dev", "on the device", "ValueError", "count", "status", "list_errors", "host_io",
                 "frame_skip", "retain_obs"):
        assert word in doc, word
    doc = TDEngine.copy_boards_dev.__doc__
    for word in ("td_copy_boards_dev", "ValueError", "list_errors", "copy_boards"):
        assert word in doc, word
    assert "td_list_errors" in TDEngine.list_errors.__doc__
    # the host-list methods point at the new ones
    assert "step_boards_dev" in TDEngine.step_boards.__doc__ and "copy_boards_dev" in TDEngine.copy_boards.__doc__
    assert "copy_boards_dev" in envs.TDVecEnv.fork_dev.__doc__
    assert "step_boards_dev" in envs.TDVecEnv.step_boards_dev.__doc__


def test_device_list_methods_do_not_bring_anything_to_the_host():
    """No .cpu(), no .item(), no numpy conversion in the two methods and their helpers."""
    import inspect
    from gym_TD import engine
    for fn in (engine.TDEngine.step_boards_dev, engine.TDEngine.copy_boards_dev, engine._dev_ids, engine._dev_words):
        text = inspect.getsource(fn)
        body = text[text.index('"""', text.index('"""') + 3) + 3:] if '"""' in text else text
        for word in (".cpu(", ".item(", ".numpy(", ".tolist(", "np.asarray"):
            assert word not in body, (fn.__name__, word)


def test_ledger_cases_under_sanitizers(tmp_path):
    """scripts/list_ledger_host.cpp: a device-list step and copy into the retained buffer with all
    boards known and with only some known, into another buffer and with NULL, random sequences
    that may never raise n_known or set retained_valid, and the check's plain arithmetic
    (td_list_check.h) -- a program of its own built with -fsanitize=address,undefined (any
    report aborts it)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "list_ledger_host")
    src = os.path.join(ROOT, "scripts", "list_ledger_host.cpp")
    cc = subprocess.run([cxx] + flags + ["-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.search(r"list_ledger: \d+ cases ok", run.stdout), run.stdout
