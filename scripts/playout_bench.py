#!/usr/bin/env python
"""Time of a random playout of k sub-steps, three ways, same build.  Needs a GPU; not part of
bench.py's metric.

    python scripts/playout_bench.py --shape 0 [--ks 4,16,64] [--burnin 64] [--rounds 3] [--calls 0]
                                    [--out profiles/playout/playout_bench.jsonl]

One process per shape (--shape indexes SHAPES): 65,536 x 10x10 TD-def, 4,096 x 10x10, 16,384 x
30x30, 16,384 x 10x10 TD-2p, and a 4,096-board device list out of 65,536 x 10x10.  Three engines on
the same seeds, each ``--burnin`` sampled steps into a rollout.  Per k, ``--rounds`` alternating
blocks per variant between one pair of device events:
  (a) playout   td_playout (the list shape: td_playout_boards_dev);
  (b) loop      k x (td_sample_actions + td_step) on a default retained engine (the list shape:
                sample_actions_boards_dev + step_boards_dev): the best existing loop;
  (c) skip      frame skip at the same k with the no-op action (k <= 16; the list shape has no
                frame-skip form): the yardstick of pure board work.
A block is ``--calls`` calls (0: about 4,096 / k sub-steps' worth, 8 at least).  Microseconds per
call, every block and the median; playout steps per second counted from steps_run (a), from the
boards a step ran on (b: every board, every sub-step -- the loop has no early stop) and from the
step counters (c).  One JSON line per k.  There is no pass mark: (a) counts as faster only where
it lies outside (b)'s own spread over its blocks."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))
from gym_TD.engine import TDEngine  # noqa: E402

# (L, boards, mode, list length or 0)
SHAPES = [(10, 65536, "def", 0), (10, 4096, "def", 0), (30, 16384, "def", 0), (10, 16384, "2p", 0), (10, 65536, "def", 4096)]
MAX_SKIP = 16


def make(L, B, mode, burnin, frame_skip=1):
    seeds = np.arange(B)
    eng = TDEngine(L, B, mode, False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=True, sample_seed=1)
    eng.reset_all()
    for i in range(burnin):
        out = eng.sample_actions(ticket=i)
        eng.step(def_act=out["def"], atk_act=out["atk"])
    if frame_skip > 1:
        eng.set_frame_skip(frame_skip)
    torch.cuda.synchronize()
    return eng


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
        sys.exit("playout_bench.py needs a GPU")
    L, B, mode, n_list = SHAPES[args.shape]
    pa, lo = make(L, B, mode, args.burnin), make(L, B, mode, args.burnin)
    ids = None
    if n_list:
        g = torch.Generator()
        g.manual_seed(2)
        ids = torch.randperm(B, generator=g)[:n_list].sort().values.to(torch.int32).to(pa.device)
    noop = torch.full((B,), 6 * L * L, dtype=torch.int64, device=pa.device)
    none = torch.full((B, 3, 8), 4, dtype=torch.int64, device=pa.device)
    ticket = [1 << 20]
    for k in [int(v) for v in args.ks.split(",")]:
        calls = args.calls or max(8, 4096 // k)
        sk = make(L, B, mode, args.burnin, k) if (k <= MAX_SKIP and not n_list) else None

        def playout(i):
            ticket[0] += k
            if ids is None:
                pa.playout(k, ticket=ticket[0])
            else:
                pa.playout_boards_dev(ids, k, ticket=ticket[0])

        def loop(i):
            for j in range(k):
                ticket[0] += 1
                if ids is None:
                    out = lo.sample_actions(ticket=ticket[0])
                    lo.step(def_act=out["def"], atk_act=out["atk"])
                else:
                    out = lo.sample_actions_boards_dev(ids, ticket=ticket[0])
                    lo.step_boards_dev(ids, def_act=out["def"], atk_act=out["atk"])

        def skip(i):
            sk.step(def_act=noop if mode != "atk" else None, atk_act=none if mode != "def" else None)

        variants = [("playout", playout), ("loop", loop)] + ([("skip", skip)] if sk is not None else [])
        for _, fn in variants:  # warm
            timed(fn, 2)
        us = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                us[name].append(timed(fn, calls if name != "loop" else max(2, calls // 4)))
        # the sub-steps a call executes: counted over a few calls of their own
        n_count, ran = 8, {}
        tot = 0
        for i in range(n_count):
            playout(i)
            r = pa._playout_buf["steps_run"]
            tot += int((r if ids is None else r[ids.long()]).sum().item())
        ran["playout"] = tot / n_count
        ran["loop"] = float((n_list or B) * k)
        if sk is not None:
            torch.cuda.synchronize()
            before = torch.from_numpy(sk.export_state()["hdr"]["steps"].astype(np.int64)).to(sk.device)
            tot = 0
            for i in range(n_count):
                skip(i)
                tot += int((sk.ep_len.to(torch.int64) - before).sum().item())
                before = torch.where(sk.done != 0, torch.zeros_like(before), sk.ep_len.to(torch.int64))
            ran["skip"] = tot / n_count
            sk.close()
        rec = {"L": L, "boards": B, "mode": mode, "list": n_list, "k": k, "calls_per_block": calls, "burnin": args.burnin,
               "kernel": pa.playout_kernel_name(), "variants": {}}
        for name, _ in variants:
            med = float(np.median(us[name]))
            rec["variants"][name] = {"us_per_call": [round(v, 2) for v in us[name]], "us_per_call_median": round(med, 2),
                                     "sub_steps_per_call": round(ran[name], 1),
                                     "playout_steps_per_s": round(ran[name] / (med * 1e-6), 1)}
        a, b = rec["variants"]["playout"], rec["variants"]["loop"]
        rec["loop_over_playout"] = round(b["us_per_call_median"] / a["us_per_call_median"], 3)
        rec["outside_loop_spread"] = bool(max(a["us_per_call"]) < min(b["us_per_call"]))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    pa.close()
    lo.close()


if __name__ == "__main__":
    main()
