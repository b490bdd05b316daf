"""The whole launch table (td_step_launch.h) on the device: every row of the step, frame-skip
and partial-step families, both observation formats.

One sweep over 40 engines of 8 boards -- L in {10, 20, 30} (kernels built for the side) and 12
(generic L), the five mode / multi-action rows, float32 and float16 -- asks on each engine for
every kernel it can launch: the step kernel of every kind the side has (td_set_step_kernel), the
frame-skip kernel where the engine is not multi-action (td_set_frame_skip(2)) and the partial
step's (td_step_boards_kernel_name).  Each row is launched once with td_kernel_timing(1) armed,
so the launch goes through the event-bound form of the shared launcher.  The tests below assert
on what the sweep recorded:

  * the name is exactly the kernel template and arguments the row stands for;
  * the name's mangled key is in exactly one kernel symbol of the built library;
  * no two different rows return the same name;
  * every timed launch returned one positive kernel time.

Nothing here is about speed."""
import numpy as np
import pytest
import torch

import test_kernel_meta as KM

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402

lib = _lib.lib
B = 8
SIDES = [10, 20, 30, 12]
ROWS = [("def", False), ("def", True), ("atk", False), ("2p", False), ("2p", True)]  # (mode, multi-action)
MODE_ARG = {"def": 0, "atk": 1, "2p": 2}
FORMATS = [(torch.float32, ""), (torch.float16, "_f16")]
STEP_STEMS = {"large": "td_step_kernel", "small": "td_step_kernel_small", "small2": "td_step_kernel_small2"}


def _empty(eng):
    """The action that changes nothing, for every board."""
    L, d, a = eng.L, None, None
    if eng.mode != "atk":
        d = np.zeros((B, 6, L, L), dtype=np.int64) if eng.multi else np.full(B, 6 * L * L, dtype=np.int64)
    if eng.mode != "def":
        a = np.full((B, 3, 8), 4, dtype=np.int64)
    return (None if d is None else torch.from_numpy(d)), (None if a is None else torch.from_numpy(a))


def _timed(eng, launch):
    """The kernel times of one launch with one event pair armed."""
    eng.kernel_timing(1)
    launch()
    return [float(t) for t in eng.kernel_times()]


@pytest.fixture(scope="module")
def sweep():
    """One record per (family, side, mode, scan, kind, format) row: the name the library
    returned, the template and arguments expected, and the times of its one timed launch."""
    rows = []
    for L in SIDES:
        lt = L if L in (10, 20, 30) else 0
        for mode, multi in ROWS:
            for dtype, fmt in FORMATS:
                seeds = list(range(700, 700 + B))
                eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, obs_dtype=dtype)
                try:
                    eng.reset_all()
                    d, a = _empty(eng)
                    args = (lt, MODE_ARG[mode])

                    def rec(family, kind, stem, scan, name, times):
                        rows.append(dict(family=family, L=L, mode=mode, multi=multi, kind=kind, fmt=fmt, stem=stem + fmt,
                                         args=args + (() if scan is None else (scan,)), name=name, times=times))

                    for kind in (("large", "small", "small2") if lt else ("large",)):
                        eng.set_step_kernel(kind)
                        rec("step", kind, STEP_STEMS[kind], multi, eng.step_kernel_name,
                            _timed(eng, lambda: eng.step(def_act=d, atk_act=a)))
                    rec("sel", None, "td_step_sel_kernel", multi, lib.td_step_boards_kernel_name(eng._h).decode(),
                        _timed(eng, lambda: eng.step_boards([5, 0, 3], def_act=d, atk_act=a)))
                    if not multi:
                        eng.set_frame_skip(2)
                        rec("skip", None, "td_skip_kernel", None, eng.step_kernel_name,
                            _timed(eng, lambda: eng.step(def_act=d, atk_act=a)))
                    torch.cuda.synchronize()
                    assert (eng.flags() == 0).all(), (L, mode, multi, fmt, eng.flags())
                finally:
                    eng.close()
    return rows


def _row_id(r):
    return (r["family"], r["L"] if r["L"] != 12 else 0, r["mode"], r["multi"], r["kind"], r["fmt"])


def test_the_sweep_covers_the_table(sweep):
    """Per format: 3 sides x 5 rows x 3 kinds + 5 generic-L rows = 50 step kernels, 4 x 5 = 20
    partial-step kernels, 4 x 3 = 12 frame-skip kernels."""
    for fmt in ("", "_f16"):
        count = {f: len({_row_id(r) for r in sweep if r["family"] == f and r["fmt"] == fmt}) for f in ("step", "sel", "skip")}
        assert count == {"step": 50, "sel": 20, "skip": 12}, (fmt, count)


def test_names_are_the_template_and_its_arguments(sweep):
    for r in sweep:
        want = "%s<%s>" % (r["stem"], ", ".join(str(x).lower() if isinstance(x, bool) else str(x) for x in r["args"]))
        assert r["name"] == want, (_row_id(r), r["name"], want)


def test_each_name_is_one_kernel_symbol_of_the_library(sweep):
    meta = KM.kernel_meta.kernels()
    for r in sweep:
        # the mangled template and arguments, as test_step_boards_meta._one builds them
        targs = "".join("Lb%dE" % int(x) if isinstance(x, bool) else "Li%dE" % x for x in r["args"])
        key = "%d%sI%sEEv" % (len(r["stem"]), r["stem"], targs)
        found = [n for n in meta if key in n]
        assert len(found) == 1, (_row_id(r), key, found)


def test_no_two_rows_share_a_name(sweep):
    by_name = {}
    for r in sweep:
        by_name.setdefault(r["name"], set()).add(_row_id(r))
    shared = {n: ids for n, ids in by_name.items() if len(ids) != 1}
    assert not shared, shared
    assert len(by_name) == 2 * (50 + 20 + 12)


def test_every_timed_launch_returned_one_positive_time(sweep):
    for r in sweep:
        assert len(r["times"]) == 1 and r["times"][0] > 0.0, (_row_id(r), r["times"])
