#!/usr/bin/env python
"""Time of a device board copy (td_copy_boards) and of the host path it replaces.  Needs a
GPU; not part of bench.py's metric.

    python scripts/copy_bench.py [--launches 50] [--warmup 10] [--burnin 64] [--host-reps 3] [--out FILE]

Copy cost, three figures per case, each over ``--launches`` TDEngine.copy_boards calls after
``--warmup`` warm-up calls, on boards ``--burnin`` steps into a random-action rollout, with
and without the observation:

  kernel  td_copy_kernel alone, from the dispatch's own timestamps (td_kernel_timing binds an
          event pair to the launch): the figure the rate and the fraction below are made of;
  host    wall time of the call on an idle stream, from entry to return (nothing is waited
          for): the id conversion, td_copy_boards' check of the ids, the copy into the pinned
          slot and the two enqueues -- O(pairs) work a caller in a tight loop pays per copy;
  call    a device event pair around the call on an idle stream: host, upload and kernel in
          series, what one isolated copy costs end to end.

The cases:

    32,768 -> 32,768 pairs at 10x10 (65,536 boards),
     8,192 ->  8,192 pairs at 30x30 (16,384 boards),
         1 ->  4,095 pairs at 10x10 (a fan-out from one root, 4,096 boards).

One JSON line per case: the three figures in microseconds (median, min), the algorithmic bytes per
pair -- header 96 B, 20 B per live enemy, 12 B per live tower, 4 L^2 B of cells, 2,504 B of
opponent stream and 48 B of hot record, each read and written, plus the 45 L^2 4-B observation
row written -- and that byte count over the kernel's median as a rate and as a fraction of the
observation store stream of the shape (scripts/obs_ceiling.hip: 5.87 TB/s at 10x10, 5.57 TB/s
at 30x30).

Host path: for the same pairs, wall time of export_state + import_state of the same boards
(td_export_state / td_import_state, both synchronous), ``--host-reps`` times, and its ratio to
one isolated device copy with the observation (the ``call`` figure).  There is no pass mark."""
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

STREAM = {10: 5.87e12, 30: 5.57e12}  # the observation store stream alone, by map side


def make(L, B, burnin):
    seeds = np.arange(B)
    eng = TDEngine(L, B, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=False)
    eng.reset_all()
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    acts = torch.randint(0, 6 * L * L + 1, (burnin, B), generator=g, device=eng.device, dtype=torch.int64)
    for k in range(burnin):
        eng.step(def_act=acts[k])
    torch.cuda.synchronize()
    return eng


def timed_copies(eng, src, dst, write_obs, args):
    """(kernel, host, call) microseconds, a list of args.launches each."""
    for _ in range(args.warmup):
        eng.copy_boards(src, dst, write_obs=write_obs)
    torch.cuda.synchronize()
    eng.kernel_timing(args.launches)
    for _ in range(args.launches):
        eng.copy_boards(src, dst, write_obs=write_obs)
    kernel = [float(v) for v in eng.kernel_times()]
    assert len(kernel) == args.launches
    eng.kernel_timing(0)
    host, call = [], []
    for _ in range(args.launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.copy_boards(src, dst, write_obs=write_obs)
        host.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    for _ in range(args.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.copy_boards(src, dst, write_obs=write_obs)
        e1.record()
        e1.synchronize()
        call.append(e0.elapsed_time(e1) * 1e3)
    return kernel, host, call


def host_path(eng, src, dst, reps):
    """export_state + import_state of the same boards: the ranges are contiguous, a fan-out
    exports its root once and imports it tiled."""
    ms = []
    fan = len(set(src.tolist())) == 1
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if fan:
            st = eng.export_state(int(src[0]), 1)
            st = {k: np.repeat(v, len(dst), axis=0) for k, v in st.items()}
        else:
            st = eng.export_state(int(src[0]), len(src))
        eng.import_state(st, int(dst[0]))
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def case(what, L, B, src, dst, args, out):
    eng = make(L, B, args.burnin)
    try:
        hdr = eng.export_state(int(src.min()), int(src.max() - src.min() + 1))["hdr"]
        n_en = float(hdr["n_en"][src - src.min()].mean())
        n_tw = float(hdr["n_tw"][src - src.min()].mean())
        state = 96 + 20 * n_en + 12 * n_tw + 4 * L * L + 2504 + 48
        obs = 45 * L * L * 4
        res = {}
        for write_obs in (True, False):
            kernel, host, call = timed_copies(eng, src, dst, write_obs, args)
            med = float(np.median(kernel))
            per_pair = 2 * state + (obs if write_obs else 0)
            rate = len(src) * per_pair / (med * 1e-6)
            res[write_obs] = float(np.median(call))
            row = {"what": what, "L": L, "boards": B, "pairs": len(src), "obs": write_obs, "launches": len(kernel),
                   "kernel_us_median": round(med, 2), "kernel_us_min": round(float(np.min(kernel)), 2),
                   "host_us_median": round(float(np.median(host)), 2), "host_us_min": round(float(np.min(host)), 2),
                   "call_us_median": round(res[write_obs], 2), "call_us_min": round(float(np.min(call)), 2),
                   "enemies_per_source": round(n_en, 2), "towers_per_source": round(n_tw, 2),
                   "bytes_per_pair": round(per_pair, 1), "TBps": round(rate / 1e12, 3),
                   "frac_of_obs_store_stream": round(rate / STREAM[L], 3)}
            print(json.dumps(row), flush=True)
            out.append(row)
        ms = host_path(eng, src, dst, args.host_reps)
        row = {"what": what + ": host path (export_state + import_state)", "L": L, "pairs": len(src),
               "ms": [round(v, 2) for v in ms], "ms_median": round(float(np.median(ms)), 2),
               "ratio_to_one_device_copy_call_with_obs": round(float(np.median(ms)) * 1e3 / res[True], 1)}
        print(json.dumps(row), flush=True)
        out.append(row)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("copy_bench.py needs a GPU")
    out = []
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    case("half to half", 10, 65536, i32(np.arange(32768)), i32(np.arange(32768, 65536)), args, out)
    case("half to half", 30, 16384, i32(np.arange(8192)), i32(np.arange(8192, 16384)), args, out)
    case("fan-out from one root", 10, 4096, i32(np.zeros(4095)), i32(np.arange(1, 4096)), args, out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in out:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
