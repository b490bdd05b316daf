"""The kernel of a skipping launch without a GPU: the rule and the resolution order of a
handle's two kinds (td_kernel_choice.h retained_kernel_kind, KernelChoice::resolve) run as a
stand-alone host program under the address and undefined-behaviour sanitizers, and the two new
functions as the headers declare them and the ctypes binding binds them."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from gym_TD import _lib
from gym_TD.engine import TDEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _decl(src, name):
    m = re.search(r"^([\w ]+?[\s*]+)%s\(([^)]*)\);" % name, src, re.M)
    assert m, "%s is not declared" % name
    args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]
    return m.group(1).strip().replace(" *", "*"), args


def test_rule_and_resolution_order_under_sanitizers(tmp_path):
    """scripts/retained_kernel_host.cpp: every boundary of the rule (one round of boards, the
    format, the map side, a generic L) for every full kind, and forced versus TD_KERNEL_AUTO for
    both kinds; any sanitizer report aborts it."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + FLAGS + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "retained_kernel_host")
    src = os.path.join(ROOT, "scripts", "retained_kernel_host.cpp")
    cc = subprocess.run([cxx] + FLAGS + ["-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"^retained_kernel: (\d+) cases ok$", run.stdout, re.M)
    assert m and int(m.group(1)) >= 300, run.stdout


def test_the_resolved_kind_stands_in_the_drop_in_header():
    """td_retained_step_kernel: in tdstep.h between td_step_kernel and td_step_kernel_name,
    whose declarations stay as they were; exported and bound."""
    src = open(os.path.join(INCLUDE, "tdstep.h")).read()
    assert _decl(src, "td_retained_step_kernel") == ("int", ["td_handle*"])
    at = src.index("int td_retained_step_kernel(td_handle* h);")
    assert src.index("int td_step_kernel(td_handle* h);") < at < src.index("td_step_kernel_name(td_handle* h);")
    assert src.index("td_step_kernel_name(td_handle* h);") < src.index("td_step_boards_kernel_name(td_handle* h);")
    fn = _lib.lib.td_retained_step_kernel  # (AttributeError: the library does not export it)
    assert fn.restype == ctypes.c_int and list(fn.argtypes) == [_lib.c_vp]
    assert fn(None) < 0 and _lib.lib.td_last_error() == b"NULL handle"


def test_the_hook_is_declared_as_a_test_hook_and_bound():
    """td_set_retained_step_kernel: a measurement hook, so not in the drop-in header; declared
    in a diag header, exported and bound, and it refuses a NULL handle."""
    assert "td_set_retained_step_kernel" not in open(os.path.join(INCLUDE, "tdstep.h")).read()
    src = open(os.path.join(INCLUDE, "td_diag_retained.h")).read()
    assert _decl(src, "td_set_retained_step_kernel") == ("int", ["td_handle*", "int"])
    for word in ("frame_skip", "copy_boards"):  # (the words the host tests keep out of the diag headers)
        assert word not in src and word not in open(os.path.join(INCLUDE, "td_diag.h")).read()
    fn = _lib.lib.td_set_retained_step_kernel
    assert fn.restype == ctypes.c_int and list(fn.argtypes) == [_lib.c_vp, ctypes.c_int]
    assert fn(None, 2) < 0 and _lib.lib.td_last_error() == b"NULL handle"


def test_engine_has_the_property_and_the_setter():
    assert isinstance(TDEngine.retained_step_kernel, property)
    assert "td_retained_step_kernel" in TDEngine.retained_step_kernel.__doc__
    assert "td_set_retained_step_kernel" in TDEngine.set_retained_step_kernel.__doc__
