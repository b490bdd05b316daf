#!/usr/bin/env python
"""Time of R random playouts per leaf board, two ways, same build.  Needs a GPU; not part of
bench.py's metric.

    python scripts/probe_bench.py --shape 0 [--ks 4,16,64] [--burnin 64] [--rounds 3] [--calls 0]
                                  [--out profiles/probe/probe_bench.jsonl]

One process per shape (--shape indexes SHAPES): 4,096 leaves x 16 replicas at 10x10 TD-def, 1,024 x
16 at 30x30 TD-def, 4,096 x 16 at 10x10 TD-2p, and 65,536 x 1 at 10x10 TD-def.  The leaves are boards
0 .. n - 1 of a handle of n x (1 + reps) boards, ``--burnin`` sampled steps into a rollout.  Per
steps value, ``--rounds`` alternating blocks per variant between one pair of device events:
  (a) probe     td_probe_boards_dev over the n leaves x reps;
  (b) scratch   the best the library offered before for the same number of playouts:
                td_copy_boards_dev of the leaves into the n x reps scratch boards of the same
                handle (no observation rows written), then td_playout_boards_dev on them.  The
                returns are not comparable (the board ids differ, and the id is in the sampling
                key); only the time and the playout steps per second are.
  reps == 1:    (b) is plain td_playout on a second handle of n boards, the cost of the private
                stream against it ((a): td_probe of every board).
A block is ``--calls`` calls (0: about 1,024 / steps, 4 at least).  Microseconds per call, every
block and the median; playout steps per second counted from steps_run.  One JSON line per steps
value.  There is no pass mark: (a) counts as faster only where all its blocks lie outside (b)'s
spread over its blocks."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))
from gym_TD.engine import TDEngine  # noqa: E402

# (L, leaves, reps, mode)
SHAPES = [(10, 4096, 16, "def"), (30, 1024, 16, "def"), (10, 4096, 16, "2p"), (10, 65536, 1, "def")]


def make(L, B, mode, leaves, burnin):
    """B boards on seeds 0 .. B - 1, the first ``leaves`` of them ``burnin`` sampled steps in."""
    seeds = np.arange(B)
    eng = TDEngine(L, B, mode, False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=True, sample_seed=1)
    eng.reset_all()
    ids = torch.arange(leaves, dtype=torch.int32, device=eng.device)
    for i in range(burnin):
        out = eng.sample_actions_boards_dev(ids, ticket=i)
        eng.step_boards_dev(ids, def_act=out["def"], atk_act=out["atk"])
    torch.cuda.synchronize()
    return eng, ids


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True)
    ap.add_argument("--ks", default="4,16,64")
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default=None, help="append the JSON lines there too")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_bench.py needs a GPU")
    L, n, reps, mode = SHAPES[args.shape]
    single = reps == 1
    B = n if single else n * (1 + reps)
    pa, leaves = make(L, B, mode, n, args.burnin)
    lo = make(L, n, mode, n, args.burnin)[0] if single else pa
    if not single:
        src = leaves.repeat_interleave(reps).contiguous()
        dst = torch.arange(n, n + n * reps, dtype=torch.int32, device=pa.device)
    ticket = [1 << 20]
    for k in [int(v) for v in args.ks.split(",")]:
        calls = args.calls or max(4, 1024 // k)

        def probe(i):
            ticket[0] += k * reps
            if single:
                return pa.probe(k, reps, ticket=ticket[0])
            return pa.probe_boards_dev(leaves, k, reps, ticket=ticket[0])

        def scratch(i):
            ticket[0] += k
            if single:
                return lo.playout(k, ticket=ticket[0])
            lo.copy_boards_dev(src, dst, write_obs=False)
            return lo.playout_boards_dev(dst, k, ticket=ticket[0])

        variants = [("probe", probe), ("scratch", scratch)]
        for _, fn in variants:  # warm
            timed(fn, 2)
        us = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                us[name].append(timed(fn, calls))
        # the sub-steps a call executes: counted over a few calls of their own
        n_count, ran = 4, {"probe": 0, "scratch": 0}
        for i in range(n_count):
            ran["probe"] += int(probe(i)["steps_run"][:n].sum().item())
            r = scratch(i)["steps_run"]
            ran["scratch"] += int((r if single else r[dst.long()]).sum().item())
        rec = {"L": L, "leaves": n, "reps": reps, "boards": B, "mode": mode, "steps": k, "calls_per_block": calls,
               "burnin": args.burnin, "kernel": pa.probe_kernel_name(), "variants": {}}
        for name, _ in variants:
            med = float(np.median(us[name]))
            rec["variants"][name] = {"us_per_call": [round(v, 2) for v in us[name]], "us_per_call_median": round(med, 2),
                                     "sub_steps_per_call": round(ran[name] / n_count, 1),
                                     "playout_steps_per_s": round(ran[name] / n_count / (med * 1e-6), 1)}
        a, b = rec["variants"]["probe"], rec["variants"]["scratch"]
        rec["scratch_over_probe"] = round(b["us_per_call_median"] / a["us_per_call_median"], 3)
        rec["probe_outside_scratch_spread"] = bool(max(a["us_per_call"]) < min(b["us_per_call"]))
        rec["probe_slower_outside_spread"] = bool(min(a["us_per_call"]) > max(b["us_per_call"]))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    assert pa.list_errors()[0] == 0 and lo.list_errors()[0] == 0  # every device list was accepted
    pa.close()
    if lo is not pa:
        lo.close()


if __name__ == "__main__":
    main()
