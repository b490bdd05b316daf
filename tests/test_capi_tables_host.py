"""The host logic td_capi.hip keeps in plain headers -- the export / import record
(td_state_rec.h), the TD_KERNEL_AUTO and write-through rules (td_kernel_choice.h), the
retained-observation ledger (td_obs_ledger.h) and the list calls' refusals (td_call_check.h) -- run
as stand-alone host programs under the address and undefined-behaviour sanitizers, and the Python
mirror of the record's layout held to the C table -- all without a GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gym_TD import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def cxx(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("probe")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + FLAGS + ["-o", str(tmp / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes")
    return cxx


def _run(cxx, tmp_path, name):
    """Build scripts/<name>_host.cpp with the sanitizers (any report aborts it), run it, and
    return its output: exit 0 and the '<name>: N cases ok' line, or the first failing case."""
    exe = str(tmp_path / (name + "_host"))
    src = os.path.join(ROOT, "scripts", name + "_host.cpp")
    cc = subprocess.run([cxx] + FLAGS + ["-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.search(r"^%s: \d+ cases ok$" % name, run.stdout, re.M), run.stdout
    return run.stdout


def test_state_record_under_sanitizers_and_python_mirror(cxx, tmp_path):
    """scripts/state_rec_host.cpp: sizes and offsets for L = 4, 10, 32, the retag on a record of
    0xFF in heap memory of exactly its bytes, td_import_state's header checks with their messages,
    the position fold.  The offsets it prints are the ones gym_TD.engine._decode_state walks."""
    out = _run(cxx, tmp_path, "state_rec")
    lines = re.findall(r"^offsets L (\d+) count (\d+):(.*) total (\d+)$", out, re.M)
    assert [int(m[0]) for m in lines] == [4, 10, 32]
    for L, count, body, total in lines:
        L, count = int(L), int(count)
        words = body.split()
        c_table = list(zip(words[0::2], map(int, words[1::2])))
        mirror, off = [], 0
        for name, dt, shape in engine._layout(count, L):
            mirror.append((name, off))
            off += count * int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        assert c_table == mirror, L
        assert int(total) == off, L
        if L == 10:
            assert off == 5944 * count
        # what _decode_state makes of a buffer of that size: every byte taken, in that order
        st = engine._decode_state(np.zeros(off, dtype=np.uint8), count, L)
        assert [k for k in st] == [n for n, _ in c_table]
        assert sum(a.nbytes for a in st.values()) == off
        assert engine._encode_state(st, count, L).nbytes == off


def test_kernel_choice_table(cxx, tmp_path):
    """scripts/kernel_choice_host.cpp: TD_KERNEL_AUTO at every round boundary of its table
    (float32 and float16, L = 10 / 20 / 30 and a generic L), and the write-through rule on both
    sides of 192 MiB."""
    _run(cxx, tmp_path, "kernel_choice")


def test_call_check_refusals(cxx, tmp_path):
    """scripts/call_check_host.cpp: what a partial step refuses of the handle's settings (frame skip
    before random_agent = 0 with auto-reset) and a device-list call of its cap and pointers (cap < 0,
    cap > B, an empty list, a NULL list, in that order), each with its whole message and the
    caller's name (td_call_check.h)."""
    _run(cxx, tmp_path, "call_check")


def test_obs_ledger_contract(cxx, tmp_path):
    """scripts/obs_ledger_host.cpp: the contract above td_retain_obs in include/tdstep.h, case by
    case -- what a full and a partial step may skip, what resets board by board make known, what
    drops it, and which freed blocks take the retention with them."""
    _run(cxx, tmp_path, "obs_ledger")
