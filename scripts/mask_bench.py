#!/usr/bin/env python
"""Time of the legal-action mask kernel (td_action_mask) on its own, and what it adds to a
step loop.  Needs a GPU; not part of bench.py's metric.

    python scripts/mask_bench.py [--launches 50] [--warmup 10] [--burnin 64] [--loop 200]

Kernel alone: device events around each of ``--launches`` launches after ``--warmup``
warm-up launches, on boards ``--burnin`` steps into a random-action rollout, for
65,536 x TD-def 10x10 (mask only, mask + code) and 16,384 x TD-def 30x30 (mask only).
Reported per shape, one JSON line each: microseconds per launch (median, min, mean), the
kernel's algorithmic bytes -- header 96 B + cell words 4 L^2 + live tower words read,
(6 L^2 + 1 padded to 16) written per output -- and that byte count over the time as a
fraction of 8 TB/s (HBM peak) and, at 10x10, of 5.87 TB/s (the store stream of the step's
observation in this board shape, README.md).  The event pair brackets one launch, so each
figure includes the launch's own start-up on an idle stream; the loop below shows what
the kernel costs behind a step.

Loop: ``--loop`` steps of 65,536 x 10x10 with and without a mask launch after every step,
alternating the two variants three times, timed with one event pair per loop: the added
time per step next to the kernel's own time says whether the mask overlaps the step's tail
or runs behind it.  There is no pass mark."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))
from gym_TD.engine import TDEngine  # noqa: E402

HBM_PEAK = 8.0e12
STREAM_10 = 5.87e12


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
    return eng, acts


def kernel_alone(L, B, code, args):
    eng, _ = make(L, B, args.burnin)
    try:
        for _ in range(args.warmup):
            eng.action_mask(code=code)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.action_mask(code=code)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        n = min(B, 4096)
        n_tw = float(eng.export_state(0, n)["hdr"]["n_tw"].mean())
        pitch = (6 * L * L + 1 + 15) & ~15
        rd, wr = 96 + 4 * L * L + 4 * n_tw, pitch * (2 if code else 1)
        med = float(np.median(us))
        rate = B * (rd + wr) / (med * 1e-6)
        out = {"what": "mask kernel alone", "L": L, "boards": B, "code": bool(code), "launches": len(us),
               "us_median": round(med, 2), "us_min": round(float(np.min(us)), 2), "us_mean": round(float(np.mean(us)), 2),
               "read_B_per_board": round(rd, 1), "written_B_per_board": wr, "towers_per_board": round(n_tw, 2),
               "TBps": round(rate / 1e12, 3), "frac_of_8TBps": round(rate / HBM_PEAK, 3)}
        if L == 10:
            out["frac_of_5.87TBps_stream"] = round(rate / STREAM_10, 3)
        print(json.dumps(out), flush=True)
        return med
    finally:
        eng.close()


def loop(args, kernel_us):
    L, B = 10, 65536
    eng, acts = make(L, B, args.burnin)
    try:
        def run(mask):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(args.loop):
                eng.step(def_act=acts[k % len(acts)])
                if mask:
                    eng.action_mask()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / args.loop
        run(True)  # warm-up of both shapes
        plain, masked = [], []
        for _ in range(3):
            plain.append(run(False))
            masked.append(run(True))
        added = float(np.median(masked) - np.median(plain))
        print(json.dumps({"what": "step loop, 65,536 x 10x10", "steps_per_loop": args.loop,
                          "us_per_step_plain": [round(v, 2) for v in plain],
                          "us_per_step_with_mask": [round(v, 2) for v in masked],
                          "added_us_per_step": round(added, 2), "mask_kernel_alone_us": round(kernel_us, 2)}), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--loop", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mask_bench.py needs a GPU")
    k10 = kernel_alone(10, 65536, False, args)
    kernel_alone(10, 65536, True, args)
    kernel_alone(30, 16384, False, args)
    loop(args, k10)


if __name__ == "__main__":
    main()
