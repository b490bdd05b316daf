#!/usr/bin/env python
"""Time of a partial step (td_step_boards) against the full step it is a part of, and against a
dedicated handle of as many boards.  Needs a GPU; not part of bench.py's metric.

    python scripts/step_boards_bench.py [--launches 50] [--warmup 10] [--burnin 64] [--out FILE]

Boards: 65,536 of TD-def 10x10 and 16,384 of 30x30, ``--burnin`` random-action steps into a
rollout (auto-reset on).  List lengths n = 64, 1,024, 4,096, 8,192, 32,768 and every board, as
sorted random subsets, and 8,192 once more unsorted.  Per n, each over ``--launches`` calls
after ``--warmup`` warm-up calls, as median / min in microseconds:

  kernel  td_step_sel_kernel alone, from the dispatch's own timestamps (td_kernel_timing);
  host    wall time of TDEngine.step_boards on an idle stream, from entry to return (nothing is
          waited for): the check of the ids, the copy into the pinned slot and the enqueues;
  call    a device event pair around one call on an idle stream: host, upload and kernel in series.

Reference 1 (n = every board): the full step's kernel forced to TD_KERNEL_LARGE on the same
handle, in the same session, the two alternating call by call -- the same board code plus one id
load.  ``ratio_to_large`` is the partial kernel's median over the large kernel's, and
``large_spread`` the large kernel's own (max - min) / median over its samples, the margin the
ratio gets.

Reference 2 (n <= 8,192): the kernel time of a full step of a handle of n boards at its AUTO
kernel, same map, same burn-in: what a dedicated small handle would cost
(``ratio_to_small_handle``).  There is no pass mark."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))
from gym_TD import _lib  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402


def make(L, B, burnin, kernel="auto"):
    seeds = np.arange(B)
    eng = TDEngine(L, B, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=False, step_kernel=kernel)
    eng.reset_all()
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    eng.acts = torch.randint(0, 6 * L * L + 1, (burnin, B), generator=g, device=eng.device, dtype=torch.int64)
    for k in range(burnin):
        eng.step(def_act=eng.acts[k])
    torch.cuda.synchronize()
    return eng


def stats(v):
    return round(float(np.median(v)), 2), round(float(np.min(v)), 2)


def timed(eng, ids, args):
    """(kernel, host, call) microseconds of step_boards(ids), a list of args.launches each."""
    acts, nb = eng.acts, len(eng.acts)
    for k in range(args.warmup):
        eng.step_boards(ids, def_act=acts[k % nb])
    torch.cuda.synchronize()
    eng.kernel_timing(args.launches)
    for k in range(args.launches):
        eng.step_boards(ids, def_act=acts[k % nb])
    kernel = [float(v) for v in eng.kernel_times()]
    assert len(kernel) == args.launches
    eng.kernel_timing(0)
    host, call = [], []
    for k in range(args.launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.step_boards(ids, def_act=acts[k % nb])
        host.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    for k in range(args.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.step_boards(ids, def_act=acts[k % nb])
        e1.record()
        e1.synchronize()
        call.append(e0.elapsed_time(e1) * 1e3)
    return kernel, host, call


def full_vs_large(eng, args):
    """Kernel times of step_boards(every board) and of the full step's large kernel, alternating."""
    acts, nb = eng.acts, len(eng.acts)
    ids = np.arange(eng.B, dtype=np.int32)
    eng.set_step_kernel("large")
    for k in range(args.warmup):
        eng.step_boards(ids, def_act=acts[k % nb])
        eng.step(def_act=acts[k % nb])
    torch.cuda.synchronize()
    eng.kernel_timing(2 * args.launches)
    for k in range(args.launches):
        eng.step_boards(ids, def_act=acts[k % nb])
        eng.step(def_act=acts[k % nb])
    t = [float(v) for v in eng.kernel_times()]
    assert len(t) == 2 * args.launches
    eng.kernel_timing(0)
    eng.set_step_kernel("auto")
    return t[0::2], t[1::2]


def small_handle(L, n, args):
    """Kernel times of a full step of a handle of n boards at its AUTO kernel."""
    eng = make(L, n, args.burnin)
    try:
        acts, nb = eng.acts, len(eng.acts)
        for k in range(args.warmup):
            eng.step(def_act=acts[k % nb])
        torch.cuda.synchronize()
        eng.kernel_timing(args.launches)
        for k in range(args.launches):
            eng.step(def_act=acts[k % nb])
        t = [float(v) for v in eng.kernel_times()]
        return t, eng.step_kernel_name
    finally:
        eng.close()


def case(L, B, args, out):
    def emit(row):
        print(json.dumps(row), flush=True)
        out.append(row)

    eng = make(L, B, args.burnin)
    try:
        name = _lib.lib.td_step_boards_kernel_name(eng._h).decode()
        rng = np.random.RandomState(7)
        sizes = [n for n in (64, 1024, 4096, 8192, 32768) if n < B] + [B]
        lists = [(n, "sorted", np.sort(rng.permutation(B)[:n]).astype(np.int32)) for n in sizes]
        lists.insert(4, (8192, "unsorted", rng.permutation(B)[:8192].astype(np.int32)))
        for n, order, ids in lists:
            kernel, host, call = timed(eng, ids, args)
            row = {"what": "step_boards", "L": L, "boards": B, "n": n, "order": order, "kernel": name,
                   "launches": len(kernel)}
            for key, v in (("kernel", kernel), ("host", host), ("call", call)):
                row[key + "_us_median"], row[key + "_us_min"] = stats(v)
            if n == B:
                sel, large = full_vs_large(eng, args)
                row["alternating_sel_us_median"], row["alternating_sel_us_min"] = stats(sel)
                row["large_us_median"], row["large_us_min"] = stats(large)
                row["large_us_max"] = round(float(np.max(large)), 2)
                row["ratio_to_large"] = round(float(np.median(sel) / np.median(large)), 4)
                row["large_spread"] = round(float((np.max(large) - np.min(large)) / np.median(large)), 4)
                row["large_kernel"] = "td_step_kernel"
            if n <= 8192 and order == "sorted":
                t, small_name = small_handle(L, n, args)
                row["small_handle_us_median"], row["small_handle_us_min"] = stats(t)
                row["small_handle_kernel"] = small_name
                row["ratio_to_small_handle"] = round(float(np.median(kernel) / np.median(t)), 3)
            emit(row)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("step_boards_bench.py needs a GPU")
    out = []
    case(10, 65536, args, out)
    case(30, 16384, args, out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in out:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
