#!/usr/bin/env python
"""Step time of the three step kernels under a retained observation, same build.
Needs a GPU; not part of bench.py's metric.

    python scripts/retained_kernel_bench.py [--burnin 64] [--warmup 20] [--loop 200] [--rounds 3]
                                            [--timed 100] [--out profiles/retained_kernel/sweep.jsonl]
                                            [--rows 0,3]

What td_kernel_choice.h retained_kernel_kind is written from.  A default TDEngine retains its
observation, so every step after the first is a skipping launch: it stores less than half the
bytes and is bound by the boards in flight, not by the store stream the TD_KERNEL_AUTO rule was
tuned on.  Per row -- TD-def 10x10 at 12,288 / 16,384 / 32,768 / 65,536 boards, TD-atk and TD-2p
10x10 at 16,384, TD-def multi-action 10x10 at 16,384, TD-2p 20x20 multi-action at 16,384, TD-def
30x30 at 16,384, then TD-atk, TD-2p and TD-def multi-action 10x10 at 65,536 and TD-2p multi-action
10x10 at 16,384 -- a process of its own holds three retained engines on the same seeds, one per
kernel, forced with set_step_kernel (which forces skipping launches too).  Each runs ``--burnin``
steps into a random-action rollout and ``--warmup`` steps warm; then ``--rounds`` times,
alternating the kernels: ``--loop`` steps between one pair of device events (microseconds per
step, launch gaps included).  Last, ``--timed`` steps with td_kernel_timing: the kernel's own
dispatch-to-end time, its median.  One JSON line per row: every block of every kernel, the
kind td_create's rules resolve for both kinds of launch, and ``switch``: the fastest kernel if
its slowest block is below the fastest block of the full-write rule's kernel, else null (the
bar a row of the rule has to clear).  There is no pass mark."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))

ROWS = [(10, 12288, "def", False), (10, 16384, "def", False), (10, 32768, "def", False), (10, 65536, "def", False),
        (10, 16384, "atk", False), (10, 16384, "2p", False), (10, 16384, "def", True), (20, 16384, "2p", True),
        (30, 16384, "def", False),
        # beyond the required rows: where the full-write rule has gone over to the large kernel
        (10, 65536, "atk", False), (10, 65536, "2p", False), (10, 65536, "def", True), (10, 16384, "2p", True)]
KERNELS = ("large", "small", "small2")
N_BUFS = 2  # pre-drawn action batches cycled by the loop (multi-action flags are 315 MB a batch)


def actions(torch, L, B, mode, multi, device):
    g = torch.Generator(device=device)
    g.manual_seed(1)
    acts = []
    for _ in range(N_BUFS):
        d = a = None
        if mode != "atk":
            d = torch.randint(0, 3, (B, 6, L, L), generator=g, device=device, dtype=torch.int64) if multi else \
                torch.randint(0, 6 * L * L + 1, (B,), generator=g, device=device, dtype=torch.int64)
        if mode != "def":
            a = torch.randint(0, 5, (B, 3, 8), generator=g, device=device, dtype=torch.int64)
        acts.append((d, a))
    return acts


def run(eng, acts, n):
    for k in range(n):
        eng.step(def_act=acts[k % N_BUFS][0], atk_act=acts[k % N_BUFS][1])


def row(L, B, mode, multi, args):
    import numpy as np
    import torch
    from gym_TD.engine import TDEngine
    if not torch.cuda.is_available():
        sys.exit("retained_kernel_bench.py needs a GPU")
    seeds = np.arange(B)
    engs, acts = {}, None
    try:
        auto = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=False)
        rule = {"full": auto.step_kernel, "retained": auto.retained_step_kernel}
        auto.close()
        for k in KERNELS:
            e = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=False, step_kernel=k)
            assert e.retain_obs and e.step_kernel == k and e.retained_step_kernel == k
            engs[k] = e
            e.reset_all()
            if acts is None:
                acts = actions(torch, L, B, mode, multi, e.device)
            run(e, acts, args.burnin + args.warmup)
        torch.cuda.synchronize()
        step_us = {k: [] for k in KERNELS}
        for _ in range(args.rounds):
            for k in KERNELS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(engs[k], acts, args.loop)
                e1.record()
                e1.synchronize()
                step_us[k].append(round(e0.elapsed_time(e1) * 1e3 / args.loop, 2))
        kern = {}
        for k in KERNELS:
            engs[k].kernel_timing(args.timed)
            run(engs[k], acts, args.timed)
            torch.cuda.synchronize()
            t = engs[k].kernel_times()
            kern[k] = {"median": round(float(np.median(t)), 2), "min": round(float(t.min()), 2), "n": int(t.size),
                       "name": engs[k].step_kernel_name}
        best = min(KERNELS, key=lambda k: max(step_us[k]))
        clear = best != rule["full"] and max(step_us[best]) < min(step_us[rule["full"]])
        return {"L": L, "boards": B, "mode": mode, "multi_action": multi, "rule": rule, "step_us": step_us,
                "step_us_median": {k: float(np.median(step_us[k])) for k in KERNELS}, "kernel_us": kern,
                "switch": best if clear else None,
                "gain": round(float(np.median(step_us[rule["full"]]) / np.median(step_us[best])), 4),
                "steps_per_block": args.loop, "burnin": args.burnin, "warmup": args.warmup}
    finally:
        for e in engs.values():
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timed", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "retained_kernel", "sweep.jsonl"))
    ap.add_argument("--rows", default=None, help="indices into ROWS, comma-separated (default: all)")
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)  # the child of one row
    args = ap.parse_args()
    if args.one is not None:
        print(json.dumps(row(*ROWS[args.one], args)), flush=True)
        return
    # one fresh process per row (this one never opens the GPU); the first row that fails ends the sweep
    picked = range(len(ROWS)) if args.rows is None else [int(i) for i in args.rows.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for i in picked:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", str(i)]
            for name in ("burnin", "warmup", "loop", "rounds", "timed"):
                cmd += ["--" + name, str(getattr(args, name))]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=240)
            if p.returncode != 0:
                sys.exit("row %d: exit status %d" % (i, p.returncode))
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
