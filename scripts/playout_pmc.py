#!/usr/bin/env python
"""Counter run of the playout kernel against frame skip, one variant per process.  Needs a GPU.

The driver (run under rocprofv3 --pmc, counters only, no tracing):

    rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES \\
              SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE -d OUT/VARIANT -o pmc --output-format csv -- \\
        python scripts/playout_pmc.py --variant VARIANT [--L 30] [--boards 16384] [--k 16] [--calls 6]

Every variant brings the same engine ``--burnin`` no-op steps into its episodes (the boards hold
the built-in attacker's enemies and no tower), then launches ``--calls`` times:
  playout       td_playout of k sub-steps, idle 0: the defender builds, every sub-step draws;
  playout_idle  the same with def_idle = 2^32 - 1: every sub-step still counts its candidates and
                draws, but the defender (almost) never acts, so the boards stay as frame skip's;
  skip          frame skip at k with the no-op: pure board work, one observation written.
Each process prints one JSON line: microseconds per call between two device events (meaningful
without the profiler only) and the towers and enemies per board at the end.
playout_idle against skip is the cost of the draw and of keeping the raw cell words; playout
against playout_idle is the work of the fuller boards.

The summary (no GPU):

    python scripts/playout_pmc.py --summarise OUT [--out profiles/playout/pmc_30x30.json]

reads OUT/<variant>/**/*counter_collection.csv and prints, per variant, the means per dispatch
of the variant's kernel over its last ``--calls`` dispatches."""
import argparse
import csv
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"playout": "td_playout_kernel", "playout_idle": "td_playout_kernel", "skip": "td_skip_kernel"}


def drive(args):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))
    from gym_TD.engine import TDEngine
    L, B, k = args.L, args.boards, args.k
    seeds = np.arange(B)
    eng = TDEngine(L, B, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=True, sample_seed=1)
    eng.reset_all()
    noop = torch.full((B,), 6 * L * L, dtype=torch.int64, device=eng.device)
    for _ in range(args.burnin):
        eng.step(def_act=noop)
    if args.variant == "skip":
        eng.set_frame_skip(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.calls):
        if args.variant == "skip":
            eng.step(def_act=noop)
        else:
            eng.playout(k, ticket=1000 + k * i, def_idle=0 if args.variant == "playout" else 2 ** 32 - 1)
    e1.record()
    torch.cuda.synchronize()
    hdr = eng.export_state()["hdr"]
    print(json.dumps({"variant": args.variant, "L": L, "boards": B, "k": k, "calls": args.calls,
                      "us_per_call": round(e0.elapsed_time(e1) * 1e3 / args.calls, 1),
                      "towers_per_board": round(float(hdr["n_tw"].mean()), 2),
                      "enemies_per_board": round(float(hdr["n_en"].mean()), 2)}), flush=True)
    eng.close()


def summarise(args):
    out = {}
    for variant, kernel in VARIANTS.items():
        rows = {}
        for path in glob.glob(os.path.join(args.summarise, variant, "**", "*counter_collection.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    if kernel in r["Kernel_Name"]:
                        rows.setdefault(int(r["Dispatch_Id"]), {"kernel": r["Kernel_Name"]})[r["Counter_Name"]] = \
                            float(r["Counter_Value"])
        last = [rows[d] for d in sorted(rows)[-args.calls:]]
        if not last:
            continue
        names = sorted(n for n in last[0] if n != "kernel")
        out[variant] = {"kernel": last[0]["kernel"], "dispatches": len(last),
                        "mean": {n: round(sum(r[n] for r in last) / len(last), 1) for n in names}}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=sorted(VARIANTS))
    ap.add_argument("--L", type=int, default=30)
    ap.add_argument("--boards", type=int, default=16384)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--summarise", default=None, help="directory with one sub-directory of counter CSVs per variant")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        summarise(args)
    elif args.variant:
        drive(args)
    else:
        ap.error("--variant or --summarise")


if __name__ == "__main__":
    main()
