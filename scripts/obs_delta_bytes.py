#!/usr/bin/env python
"""How many observation bytes a step has to write when the buffer keeps the last step's
(td_retain_obs): the CPU prediction behind the retained observation, no GPU.

    python scripts/obs_delta_bytes.py [--boards 4800] [--burnin 1200] [--steps 40] [--seed 0]

Runs TD-def 10x10 on the C restatement (oracle.td_cpu.Batch) in bench.py's steady state:
explicit resets staggered over the burn-in (board i at step i modulo 1,200), uniform random
defender actions in [0, 601), auto-reset on.  Over the steps after the burn-in it compares
every board's float32 observation with the previous step's and prints, per board and step,

* the bytes that actually differ;
* the bytes the conservative class rule writes -- the dirty classes of td_board.h (OD_*),
  derived from what the step kernel knows: an episode end, channel 5, the tower planes,
  channels 21-24, an enemy before or after, and the always-dirty channels -- at the
  granularity of the writer's 128-B-aligned 1-KB windows (write_obs_lines), and at 128-B
  lines;
* the share of boards with an enemy, with changed tower planes, and that ended an episode;
* the windows written per board and step when the enemy class is dirty whenever the board had
  or has an enemy (the rule up to the "enemy touched" bit), when it is dirty only if a byte of
  the 16 enemy planes changed (what the touched bit of td_step_obs.h obs_dirty comes to, see
  below), and the windows that hold any changed byte at all.

The rule is asserted never to miss a changed byte: every differing byte lies in a window
(and a line) the rule writes.

``--event-envs N`` (default 160; 0 skips it) then steps N envs of the Python restatement
(oracle.td_oracle, tests/enemyclean.py's watcher) for ``--event-steps`` steps with the default
config and counts, over the board-steps after step 300 on which the enemy class was dirty under
the old rule, what the kernel's bit sees: a summon, a sort that moved an enemy, a shot that
landed, an enemy that entered a new cell -- each alone, none of them (a quiet step), how often
the planes were in fact unchanged, and the steps without an event whose planes changed
(asserted to be none)."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from oracle import td_cpu as C  # noqa: E402

L, NCH, PERIOD = 10, 45, 1200
Q = L * L // 4            # 16-B units (quads of cells) per plane
N4 = NCH * Q              # ... per board
UB, UPL, WIN = 16, 8, 64  # bytes per unit, units per 128-B line, units per window

STATIC, LP, TOWER, COST, ENEMY, ALWAYS = 1, 2, 4, 8, 16, 32


def dirty_class(ch):
    return LP if ch == 5 else STATIC if ch <= 10 else ALWAYS if ch <= 13 else TOWER if ch <= 20 else \
        COST if ch <= 24 else ENEMY if ch <= 40 else ALWAYS


UNIT_CLASS = np.array([dirty_class(u // Q) for u in range(N4)], dtype=np.uint8)


def group_classes(mis, size):
    """Per group of `size` stream units (windows: 64, lines: 8) of a board that starts `mis`
    units into its line: the classes the group overlaps, and each unit's group."""
    grp = (np.arange(N4) + mis) // size
    cls = np.zeros(grp[-1] + 1, dtype=np.uint8)
    np.bitwise_or.at(cls, grp, UNIT_CLASS)
    return cls, grp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=4800)
    ap.add_argument("--burnin", type=int, default=1200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--event-envs", type=int, default=160)
    ap.add_argument("--event-steps", type=int, default=700)
    a = ap.parse_args()
    B = a.boards
    seeds = a.seed + np.arange(B)
    bt = C.Batch(L, B, "def", 1, seeds, seeds)
    rng = np.random.RandomState(a.seed)
    idx = np.arange(B)
    tabs = {size: [group_classes(m, size) for m in range(UPL)] for size in (WIN, UPL)}
    mis = (idx * N4) % UPL
    for k in range(a.burnin):
        if 0 < k < PERIOD:
            m = (idx % PERIOD) == k
            if m.any():
                bt.reset(m)
        bt.step(rng.randint(0, 6 * L * L + 1, size=B).astype(np.int64))
    prev = bt.obs()
    cur = np.empty_like(prev)
    tot = {"differ": 0, WIN: 0, UPL: 0, "enemy": 0, "tower": 0, "done": 0, "kept": 0, "same": 0, "w_old": 0, "w_new": 0,
           "w_any": 0}
    for k in range(a.steps):
        _, done = bt.step(rng.randint(0, 6 * L * L + 1, size=B).astype(np.int64), obs=cur)
        done = done.astype(bool)
        changed = (prev.view(np.uint32) != cur.view(np.uint32)).reshape(B, N4, 4)
        tot["differ"] += int(changed.sum()) * 4
        enemy = prev[:, 25:41].reshape(B, -1).any(axis=1) | cur[:, 25:41].reshape(B, -1).any(axis=1)
        tower = (prev[:, 14:21] != cur[:, 14:21]).reshape(B, -1).any(axis=1)
        dirty = np.full(B, ALWAYS, dtype=np.uint8)
        dirty[(prev[:, 5] != cur[:, 5]).reshape(B, -1).any(axis=1)] |= LP
        dirty[tower] |= TOWER
        dirty[(prev[:, 21:25] != cur[:, 21:25]).reshape(B, -1).any(axis=1)] |= COST
        dirty[enemy] |= ENEMY
        dirty[done] = 63  # a new episode: every class
        # the same with the enemy class dirty only where a byte of the enemy planes changed
        en_changed = (prev[:, 25:41].view(np.uint32) != cur[:, 25:41].view(np.uint32)).reshape(B, -1).any(axis=1)
        dirty_new = dirty.copy()
        dirty_new[enemy & ~en_changed & ~done] &= ~np.uint8(ENEMY)
        tot["kept"] += int((enemy & ~done).sum())
        tot["same"] += int((enemy & ~done & ~en_changed).sum())
        tot["enemy"] += int(enemy.sum())
        tot["tower"] += int((tower & ~done).sum())
        tot["done"] += int(done.sum())
        uchg = changed.any(axis=2)
        for b in range(B):
            for size in (WIN, UPL):
                cls, grp = tabs[size][mis[b]]
                written = (cls & dirty[b]) != 0
                tot[size] += int(written[grp].sum()) * UB
                assert not (uchg[b] & ~written[grp]).any(), ("the rule missed a changed byte", k, b, size)
            cls, grp = tabs[WIN][mis[b]]
            tot["w_old"] += int(((cls & dirty[b]) != 0).sum())
            new = (cls & dirty_new[b]) != 0
            tot["w_new"] += int(new.sum())
            assert not (uchg[b] & ~new[grp]).any(), ("the changed-planes rule missed a changed byte", k, b)
            tot["w_any"] += len(np.unique(grp[uchg[b]]))
        prev, cur = cur, prev
    n = float(B * a.steps)
    print("boards %d, burn-in %d, steps %d: per board and step" % (B, a.burnin, a.steps))
    print("  boards with an enemy before or after   %5.1f %%" % (100 * tot["enemy"] / n))
    print("  boards whose tower planes changed      %5.1f %%" % (100 * tot["tower"] / n))
    print("  boards that ended an episode           %5.2f %%" % (100 * tot["done"] / n))
    print("  bytes that differ                      %6.0f B of %d" % (tot["differ"] / n, N4 * UB))
    print("  class rule, 1-KB line-aligned windows  %6.0f B (%.0f %%)" % (tot[WIN] / n, 100 * tot[WIN] / n / (N4 * UB)))
    print("  class rule, 128-B lines                %6.0f B (%.0f %%)" % (tot[UPL] / n, 100 * tot[UPL] / n / (N4 * UB)))
    print("  enemy class dirty (old rule), episode kept  %5.1f %%; of those, 16 enemy planes byte-identical %5.1f %%"
          % (100 * tot["kept"] / n, 100.0 * tot["same"] / max(tot["kept"], 1)))
    print("  windows written, enemy class dirty with an enemy before or after   %5.2f" % (tot["w_old"] / n))
    print("  windows written, enemy class dirty only when an enemy plane changed %5.2f" % (tot["w_new"] / n))
    print("  windows that hold any changed byte                                  %5.2f" % (tot["w_any"] / n))
    bt.close()
    if a.event_envs > 0:
        events(a.event_envs, a.event_steps, a.seed)


def events(envs, steps, seed, after=300):
    """The kernel's enemy-touched rule on the Python restatement (module docstring)."""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import enemyclean as E
    from oracle import td_oracle as O
    tr = E.Trace(L, envs, "def", False, steps, seed0=seed, act_seed=seed, cfg=O.Config(), hp=O.Hyper())
    ev = tr.ev[after:]
    dirty = ((ev & E.ENDED) == 0) & (((ev & E.ENEMY) != 0) | (tr.n_en[after - 1:-1] > 0))
    touch, planes = ev & E.TOUCH, (ev & E.PLANES) != 0
    nd = int(dirty.sum())
    print("Python restatement, %d envs, steps %d-%d: %d board-steps, %d with the enemy class dirty under the old rule"
          % (envs, after, steps, ev.size, nd))
    for name, bit in (("summon", E.SUMMON), ("shot", E.SHOT), ("move", E.MOVE), ("sort", E.SORT)):
        print("  %-6s alone %6d" % (name, int((dirty & (touch == bit)).sum())))
    quiet = dirty & (touch == 0)
    print("  quiet (none of the four) %6d = %.1f %% of the dirty board-steps; planes byte-identical on %.1f %%"
          % (int(quiet.sum()), 100.0 * quiet.sum() / max(nd, 1), 100.0 * (dirty & ~planes).sum() / max(nd, 1)))
    missed = int((quiet & planes).sum())
    print("  quiet steps whose enemy planes changed: %d" % missed)
    assert missed == 0


if __name__ == "__main__":
    main()
