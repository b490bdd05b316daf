#!/usr/bin/env python
"""The device-list calls (td_step_boards_dev, td_copy_boards_dev) against the host-list calls
(td_step_boards, td_copy_boards) for the same lists, in one process.  Needs a GPU; not part of
bench.py's metric.

    python scripts/board_lists_dev_bench.py [--launches 50] [--warmup 10] [--burnin 64] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/board_lists_dev_bench.py --launches 20

Shapes: a step of n = 4,096 and n = 65,536 boards of 65,536 x 10x10 and of n = 8,192 of 16,384 x
30x30 (sorted random subsets); a copy of 32,768 pairs at 10x10 and of 8,192 pairs at 30x30; the
4,095-child fan-out at 10x10.  Per shape and form, each over ``--launches`` calls after
``--warmup`` warm-up calls, as median / min in microseconds:

  kernel  the consumer kernel alone (td_step_sel_kernel / td_step_list_kernel, td_copy_kernel /
          td_copy_list_kernel), from the dispatch's own timestamps (td_kernel_timing);
  host    wall time of the engine method on an idle stream, from entry to return.  Host lists
          are int32 numpy arrays, device lists int32 device tensors: the cheapest way in of each;
  wall    wall time from entry until the stream is idle again (the call, then a synchronize).

The check kernel (td_list_check_kernel) has no event pair of its own: its time is read from the
second form of the command above (the kernel trace's per-kernel statistics).  The baseline is
the host-list entry points in the same run.  There is no pass mark."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))
from gym_TD.engine import TDEngine  # noqa: E402


def make(L, B, burnin):
    seeds = np.arange(B)
    eng = TDEngine(L, B, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=False)
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


def timed(eng, call, args):
    """(kernel, host, wall) microseconds of call(k), a list of args.launches each."""
    for k in range(args.warmup):
        call(k)
    torch.cuda.synchronize()
    eng.kernel_timing(args.launches)
    for k in range(args.launches):
        call(k)
    kernel = [float(v) for v in eng.kernel_times()]
    assert len(kernel) == args.launches
    eng.kernel_timing(0)
    host, wall = [], []
    for k in range(args.launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(k)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append((t1 - t0) * 1e6)
        wall.append((t2 - t0) * 1e6)
    return kernel, host, wall


def emit(out, what, form, L, B, n, eng, call, args):
    kernel, host, wall = timed(eng, call, args)
    row = {"what": what, "form": form, "L": L, "boards": B, "n": n, "launches": len(kernel)}
    for key, v in (("kernel", kernel), ("host", host), ("wall", wall)):
        row[key + "_us_median"], row[key + "_us_min"] = stats(v)
    print(json.dumps(row), flush=True)
    out.append(row)


def case(L, B, steps, copies, fanout, args, out):
    eng = make(L, B, args.burnin)
    try:
        acts, nb = eng.acts, len(eng.acts)
        rng = np.random.RandomState(7)
        for n in steps:
            ids = np.sort(rng.permutation(B)[:n]).astype(np.int32)
            dev = torch.from_numpy(ids).to(eng.device)
            emit(out, "step", "host", L, B, n, eng, lambda k: eng.step_boards(ids, def_act=acts[k % nb]), args)
            emit(out, "step", "device", L, B, n, eng, lambda k: eng.step_boards_dev(dev, def_act=acts[k % nb]), args)
        pairs = [("copy", n, np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)) for n in copies]
        if fanout:
            pairs.append(("fan-out", fanout, np.zeros(fanout, dtype=np.int32), np.arange(1, fanout + 1, dtype=np.int32)))
        for what, n, src, dst in pairs:
            ds, dd = torch.from_numpy(src).to(eng.device), torch.from_numpy(dst).to(eng.device)
            emit(out, what, "host", L, B, n, eng, lambda k: eng.copy_boards(src, dst), args)
            emit(out, what, "device", L, B, n, eng, lambda k: eng.copy_boards_dev(ds, dd), args)
        assert eng.list_errors() == (0, None)
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
        sys.exit("board_lists_dev_bench.py needs a GPU")
    out = []
    case(10, 65536, [4096, 65536], [32768], 4095, args, out)
    case(30, 16384, [8192], [8192], 0, args, out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in out:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
