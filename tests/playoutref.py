"""Shared pieces of the playout tests (tests/test_playout_ref.py on the CPU oracle,
tests/test_gpu_playout.py on the device): the anchor cases, the crowd configs, and the reference
run of a case -- gym_TD.sampling.reference_playout on oracle envs, with the event ledger the CPU
test holds to its floors.  Not a test module."""
import numpy as np

import cfgspace
import maskutil as M
from gym_TD import sampling as S
from oracle import td_oracle as O

SAMPLE_SEED = 7
SHIFT_TICKET = 1 << 20  # the warm-up playouts of run_case
MODES = {"def": O.MODE_DEF, "atk": O.MODE_ATK, "2p": O.MODE_2P}

# Short episodes that end from both causes: 23 steps at most, and a base that falls after three
# leaks; money and cool-downs on both sides (maskutil.RICH / ATK), so that every operation class,
# idle draws and sub-steps with nothing legal occur.
# Builds are dear and upgrades cheap, so that the level-ups and destructs, a handful among hundreds
# of build candidates otherwise, are often all that is legal; fast enemies reach the base.
_ANCHOR = dict(base_LP=2, attacker_cost_init_rate=3, attacker_cost_final_rate=6, enemy_speed=[[1.2, 1.2]] * 4,
               tower_cost=[[25, 4], [30, 5], [35, 6], [28, 5]])
# k: the longest playout (and the modulus of the warm-up); the rounds cycle through KS, so that an
# episode restarted at a playout's end does not meet the step limit at the same sub-step position
# again and again.
KS = (8, 3, 5, 7, 2, 6, 4)
ANCHOR_CASES = [
    dict(name="def", mode="def", L=10, n=12, k=8, rounds=12, idle=0.3, seed0=500),
    dict(name="atk", mode="atk", L=10, n=12, k=8, rounds=12, idle=0.3, seed0=500),
    dict(name="2p", mode="2p", L=10, n=12, k=8, rounds=12, idle=0.3, seed0=500),
]


def round_plan(case):
    """[(k, ticket)] of the case's rounds: k cycles through KS, the tickets follow on one another."""
    plan, t = [], 0
    for r in range(case["rounds"]):
        k = KS[r % len(KS)]
        plan.append((k, t))
        t += k
    return plan


def anchor_config():
    return M.config(M.RICH, M.ATK, **_ANCHOR), M.hyper(max_episode_steps=23)


# One TD-def case under a swarm config (the built-in attacker's clusters of eight) and one TD-2p
# case under a fortress config (the sampled defender builds up to the capacity): cfgspace's
# regimes, with the fields that decide how fast a crowd forms pinned.
CROWD_CASES = [("def", "swarm", 11), ("2p", "fortress", 5)]
CROWD_ROUNDS = 6
_CROWD_PIN = {
    "swarm": dict(attacker_action_interval=1, base_LP=10 ** 6, attacker_init_cost=400.0, max_cost=1000.0,
                  enemy_speed=[[0.02, 0.02]] * 4),
    "fortress": dict(defender_action_interval=1, tower_distance=0, defender_init_cost=900.0, max_cost=1000.0,
                     tower_cost=[[1.25, 2.5]] * 4, base_LP=10 ** 6, tower_destruct_return=0.5),
}


def crowd_config(regime, seed):
    d = cfgspace.draw(seed, regime)
    d.update(_CROWD_PIN[regime])
    return O.Config(**d), M.hyper(max_episode_steps=200)


def new_ledger():
    return {"build": 0, "lvup": 0, "destruct": 0, "summon": 0, "idle_fired": 0, "nothing_legal": 0,
            "ends": {"base": set(), "limit": set()}, "top_enemies": 0, "top_towers": 0}


def record(led, res, env, L):
    """One playout's events into the ledger."""
    NC = L * L
    for ev in res["events"]:
        if ev["def"] is not None:
            led[("build", "build", "build", "build", "lvup", "destruct")[ev["def"] // NC]] += 1
        if ev["atk"] is not None:
            led["summon"] += 1
        for side in ("def", "atk"):
            n = ev[side + "_n"]
            if n is not None and ev[side] is None:
                led["idle_fired" if n > 0 else "nothing_legal"] += 1
    if res["done"]:
        st = M.oracle_state(env)
        led["ends"]["limit" if st["base_LP"] > 0 else "base"].add(res["steps_run"])


def play(envs, seeds_b, L, cfg, hp, mode, k, ticket, idle, led=None, cap=True):
    """reference_playout of every env (board id = its index), auto-reset mirrored: a finished env
    starts its next episode.  Returns the per-board results."""
    out = []
    for b, env in enumerate(envs):
        res = S.reference_playout(env, M.oracle_state, L, cfg, hp, mode, SAMPLE_SEED, ticket, b, k, idle, idle, cap=cap)
        if led is not None:
            record(led, res, env, L)
            st = M.oracle_state(env)
            led["top_enemies"] = max(led["top_enemies"], len(st["enemies"]))
            led["top_towers"] = max(led["top_towers"], len(st["towers"]))
        if res["done"]:
            M.reset_ok(env)
        out.append(res)
    return out


def run_case(case, led=None):
    """The anchor case on the CPU oracle: its rounds of playouts (round_plan)."""
    cfg, hp = anchor_config()
    seeds, envs = M.ok_seeds(case["L"], case["n"], case["seed0"], MODES[case["mode"]], cfg=cfg, hp=hp)
    # board b starts b mod k sub-steps into its episode: episodes end at every sub-step position
    for b, env in enumerate(envs):
        if b % case["k"]:
            res = S.reference_playout(env, M.oracle_state, case["L"], cfg, hp, case["mode"], SAMPLE_SEED, SHIFT_TICKET, b,
                                      b % case["k"], case["idle"], case["idle"])
            if res["done"]:
                M.reset_ok(env)
    rounds = [play(envs, seeds, case["L"], cfg, hp, case["mode"], k, t, case["idle"], led) for k, t in round_plan(case)]
    return {"seeds": np.asarray(seeds), "cfg": cfg, "hp": hp, "rounds": rounds, "envs": envs}
