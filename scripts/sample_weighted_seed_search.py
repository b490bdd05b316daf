#!/usr/bin/env python3
"""Which sample_seed lets the sampler-driven run of tests/test_gpu_sample_weighted.py reach its
floors -- on the CPU oracle alone, no GPU.

    python scripts/sample_weighted_seed_search.py [seed ...]        (default: 1 .. 8)

The test's case 1 drives an engine for 80 steps with TDEngine.sample_weighted alone.  This script
plays the same run with oracle envs (the engine's seeds 500 + b, failed layout draws redrawn from
the same stream as TDEngine.reset_all and the auto-reset do; L = 7: the two hand layouts) and
gym_TD.sampling.reference_sample_weighted over gym_TD.masks.reference_masks, with the test's own
weights (tests/sampleweightedutil.py), and prints per seed and shape whether every floor is
reached: each of the six defender operations and the no-op chosen, a compared board (step % 10
== 0) with a closed cool-down, a summon and a "nothing" for the attacker, an episode end.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gym-td_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import maskutil as M  # noqa: E402
import sampleweightedutil as W  # noqa: E402
from gym_TD import sampling as S  # noqa: E402
from gym_TD.masks import reference_masks  # noqa: E402
from oracle import td_oracle as O  # noqa: E402

SHAPES = [("def", 10, 128), ("atk", 10, 64), ("2p", 20, 32), ("def", 30, 16), ("def", 7, 32), ("def", 32, 8)]
STEPS, EPISODE = 80, 60
ROADS_7 = ([[(3, c) for c in range(7)]],
           [[(1, c) for c in range(7)], [(5, 0), (5, 1), (5, 2), (5, 3), (4, 3), (3, 3), (2, 3)] + [(1, c) for c in range(3, 7)]])


class Twin(O.Env):
    """An env that restarts as the engine's boards do."""
    roads7 = None

    def reset(self):
        if self.roads7 is not None:  # tests/test_gpu_action_mask.py _restart_7
            self.num_roads = len(self.roads7)
            self._board = O.Board(self.L, self.num_roads, None, self.cfg, self.hp, roads=[list(r) for r in self.roads7],
                                  enemy_cap=self.enemy_cap, tower_cap=self.tower_cap, refused=self.refused)
            self.attacker_cd = self.defender_cd = 0
            return self._board.get_states()
        while True:
            try:
                return O.Env.reset(self)
            except O.RoadGenError:
                pass


def run(mode, L, B, seed):
    cfg = M.config(M.RICH) if mode == "def" else M.config(M.RICH, M.ATK)
    hp = M.hyper(False, max_episode_steps=EPISODE)
    omode = {"def": O.MODE_DEF, "atk": O.MODE_ATK, "2p": O.MODE_2P}[mode]
    envs = []
    for b in range(B):
        cls = type("Twin7", (Twin,), {"roads7": ROADS_7[b % 2]}) if L == 7 else Twin
        envs.append(cls(L, omode, 1, 500 + b, 500 + b, cfg, hp, road_attempts=M.ROAD_ATTEMPTS))
    NC = L * L
    seen = {"ops": np.zeros(7, dtype=int), "closed": 0, "summons": 0, "nothing": 0, "done": 0}
    for k in range(STEPS):
        dw, aw = W.run_weights(k, B, L, mode)
        for b, env in enumerate(envs):
            st = M.oracle_state(env)
            dm, _, am = reference_masks(st, L, cfg, hp, mode, False)
            d, a, _, _ = S.reference_sample_weighted(dm, am, None if dw is None else dw[b], None if aw is None else aw[b],
                                                     seed, k, b, L)
            kw = {}
            if mode != "atk":
                kw["def_act"] = d
                seen["ops"][d // NC] += 1
                seen["closed"] += int(k % 10 == 0 and st["defender_cd"] > 1)
            if mode != "def":
                kw["atk_act"] = a
                seen["summons" if (a[:, 0] != 4).any() else "nothing"] += 1
            _, _, done, _ = env.step(**kw)
            if done:
                seen["done"] += 1
                env.reset()
    ok = seen["done"] > 0
    if mode != "atk":
        ok = ok and (seen["ops"] > 0).all() and seen["closed"] > 0
    if mode != "def":
        ok = ok and seen["summons"] > 0 and seen["nothing"] > 0
    return ok, seen


def main():
    seeds = [int(x) for x in sys.argv[1:]] or list(range(1, 9))
    good = []
    for seed in seeds:
        all_ok = True
        for mode, L, B in SHAPES:
            ok, seen = run(mode, L, B, seed)
            print("seed %d %s L=%d B=%d: %s %r" % (seed, mode, L, B, "ok" if ok else "MISSES", seen), flush=True)
            all_ok = all_ok and ok
        if all_ok:
            good.append(seed)
    print("seeds that reach every floor:", good)


if __name__ == "__main__":
    main()
