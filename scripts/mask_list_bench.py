#!/usr/bin/env python
"""Time of the list form of the legal-action masks (td_action_mask_boards[_dev],
td_mask_list_kernel) next to the full call (td_action_mask), and what the partial refresh
saves a search iteration of TDVecEnv(action_mask=True).  Needs a GPU; not part of bench.py's
metric; no pass mark.

    python scripts/mask_list_bench.py [--launches 50] [--warmup 10] [--burnin 64] [--iters 200]
                                      [--section lists10|lists30|identity|search] [--libs W=PATH ...]

Without --section the sections run one after another, each in a child process of its own under
its own time limit; the first that fails or runs out of time ends the run.  One JSON line per
figure, boards --burnin steps into a random-action rollout.

lists10 / lists30: n = 256 / 4,096 / 16,384 named of 65,536 x TD-def 10x10 (mask; mask + code)
and n = 1,024 of 16,384 x 30x30, host and device form, a sorted random subset.  Per figure
--launches launches after --warmup warm-ups, two ways: "call_us" -- a device-event pair around
each single call on an idle stream (the isolated call: upload or check kernel, launch start-up
and kernel), and "stream_us" -- one event pair around all the calls issued back to back, per
call (what a call costs behind other work: the kernels' own time, or the rate at which the host
can issue them, whichever is larger).  The full call is timed the same way beside them.

identity: n = B with the identity list against td_mask_kernel at the same shape, for the
library as built and for every library given with --libs (builds with another number of list
entries per workgroup: ``make -C gym-td_amd/csrc EXTRA=-DTD_MASK_LIST_WAVES=8 BUILD=../build_w8
OUT=../lib/libtdstep_w8.so``), each in its own child process.

search: 65,536 x TD-2p 10x10, action_mask=True; per iteration fork_dev of one root into 4,095
children and step_boards_dev of the 4,096; wall time per iteration over --iters iterations,
three times.  Uses TDVecEnv's public calls only, so the same file times the parent commit
(PYTHONPATH=<parent>/gym-td_amd)."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("TD_BENCH_PKG", os.path.join(HERE, "gym-td_amd"))
LIMITS = {"lists10": 240, "lists30": 180, "identity": 120, "search": 240}  # seconds per section


def out(**kw):
    print(json.dumps(kw), flush=True)


def make(L, B, burnin, mode="def"):
    import numpy as np
    import torch
    from gym_TD.engine import TDEngine
    seeds = np.arange(B)
    eng = TDEngine(L, B, mode, False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=False)
    eng.reset_all()
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    acts = torch.randint(0, 6 * L * L + 1, (burnin, B), generator=g, device=eng.device, dtype=torch.int64)
    for k in range(burnin):
        eng.step(def_act=acts[k])
    torch.cuda.synchronize()
    return eng


def timed(call, args):
    """(median, min of the isolated calls; per-call time of the calls issued back to back), in us."""
    import numpy as np
    import torch
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.launches):
        call()
    e1.record()
    e1.synchronize()
    return round(float(np.median(us)), 2), round(float(np.min(us)), 2), round(e0.elapsed_time(e1) * 1e3 / args.launches, 2)


def lists(L, B, ns, codes, args):
    import numpy as np
    import torch
    eng = make(L, B, args.burnin)
    try:
        kernel = eng.action_mask_boards_kernel_name()
        for code in codes:
            med, lo, stream = timed(lambda: eng.action_mask(code=code), args)
            out(what="full call", L=L, boards=B, code=code, call_us=med, call_us_min=lo, stream_us=stream,
                kernel="td_mask_kernel<%d>" % L)
            for n in ns:
                ids = np.sort(np.random.RandomState(n).permutation(B)[:n]).astype(np.int32)
                dev = torch.from_numpy(ids).to(eng.device)
                for form, call in (("host", lambda: eng.action_mask_boards(ids, code=code)),
                                   ("device", lambda: eng.action_mask_boards_dev(dev, code=code))):
                    m, lo_n, s = timed(call, args)
                    out(what="list call", form=form, L=L, boards=B, n=n, code=code, call_us=m, call_us_min=lo_n,
                        stream_us=s, call_vs_full=round(m / med, 3), stream_vs_full=round(s / stream, 3), kernel=kernel)
        assert eng.list_errors() == (0, None)
    finally:
        eng.close()


def identity(args):
    import numpy as np
    import torch
    from gym_TD import _lib
    for L, B in ((10, 65536), (30, 16384)):
        eng = make(L, B, args.burnin)
        try:
            med, lo, stream = timed(lambda: eng.action_mask(), args)
            dev = torch.arange(B, dtype=torch.int32, device=eng.device)
            ids = np.arange(B, dtype=np.int32)
            md, lod, sd = timed(lambda: eng.action_mask_boards_dev(dev), args)
            mh, loh, sh = timed(lambda: eng.action_mask_boards(ids), args)
            out(what="identity list, n = B", lib=os.path.basename(_lib.LIB_PATH), entries_per_workgroup=args.label, L=L,
                boards=B, full_call_us=med, full_stream_us=stream, device_call_us=md, device_stream_us=sd,
                host_call_us=mh, host_stream_us=sh, device_stream_vs_full=round(sd / stream, 3),
                host_stream_vs_full=round(sh / stream, 3))
        finally:
            eng.close()


def search(args):
    import numpy as np
    import torch
    from gym_TD import envs as E
    L, B, K = 10, 65536, 4096
    env = E.TDVecEnv(L, B, "2p", seed=0, action_mask=True, info=False)
    try:
        env.reset()
        dev = env.engine.device
        g = torch.Generator(device=dev)
        g.manual_seed(2)
        full = {"Defender": torch.randint(0, 6 * L * L + 1, (B,), generator=g, device=dev, dtype=torch.int64),
                "Attacker": torch.randint(0, 5, (B, 3, 8), generator=g, device=dev, dtype=torch.int64)}
        for _ in range(args.burnin):
            env.step(full)
        leaves = torch.from_numpy(np.sort(np.random.RandomState(3).permutation(B)[:K]).astype(np.int32)).to(dev)
        src, dst = leaves[:1].repeat(K - 1).contiguous(), leaves[1:].contiguous()

        def run(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                env.fork_dev(src, dst)
                env.step_boards_dev(leaves, full)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / n
        run(20)
        us = [round(run(args.iters), 2) for _ in range(3)]
        partial = hasattr(env.engine, "refresh_action_mask")
        out(what="search iteration: fork_dev of 4,095 + step_boards_dev of 4,096 of 65,536 x TD-2p 10x10, action_mask=True",
            iterations=args.iters, us_per_iteration=us, us_median=float(np.median(us)), partial_refresh=partial,
            package=PKG)
        assert env.engine.list_errors() == (0, None)
    finally:
        env.close()


def child(section, args, env=None, label=""):
    cmd = [sys.executable, os.path.abspath(__file__), "--section", section, "--launches", str(args.launches),
           "--warmup", str(args.warmup), "--burnin", str(args.burnin), "--iters", str(args.iters), "--label", label]
    try:
        rc = subprocess.run(cmd, env=env, timeout=LIMITS[section]).returncode
    except subprocess.TimeoutExpired:
        sys.exit("%s: no result within %d s; nothing more is started" % (section, LIMITS[section]))
    if rc != 0:
        sys.exit("%s: exit status %d; nothing more is started" % (section, rc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--section", choices=sorted(LIMITS))
    ap.add_argument("--only", nargs="*", default=None, help="the sections of a run without --section")
    ap.add_argument("--libs", nargs="*", default=[], help="identity: W=PATH, other builds of the library")
    ap.add_argument("--label", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.section is None:  # the parent: starts the children, never touches the GPU itself
        for section in args.only or ("lists10", "lists30", "identity", "search"):
            if section != "identity":
                child(section, args)
                continue
            child(section, args, label="as built")
            for spec in args.libs:
                w, path = spec.split("=", 1)
                child(section, args, env=dict(os.environ, TDSTEP_LIB=os.path.abspath(path)), label=w)
        return
    sys.path.insert(0, PKG)
    import torch
    if not torch.cuda.is_available():
        sys.exit("mask_list_bench.py needs a GPU")
    if args.section == "lists10":
        lists(10, 65536, (256, 4096, 16384), (False, True), args)
    elif args.section == "lists30":
        lists(30, 16384, (1024,), (False,), args)
    elif args.section == "identity":
        identity(args)
    else:
        search(args)


if __name__ == "__main__":
    main()
