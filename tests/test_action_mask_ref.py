"""gym_TD.masks.reference_masks against brute force on the CPU oracle (no GPU).

The mask says what the next step would do with an action "if it were the only thing asked
of that side".  Brute force: copy the oracle env, step it with exactly that action, and
read info['RealAction'] / ['FailCode'].  The runs are driven by a policy that samples from
the reference masks only, so every action it chose must also have been executed.

The defender's fail code, which the step reports only while the cool-down gate is open, is
brute-forced by calling the board's operation itself on a copy.  An attacker summon
counts as executed when its road reports fail code 0 and the first slot kept its type: the
oracle's (and the reference's) RealAction merely echoes the input while the cool-down
blocks or the road does not exist, and FailCode has no entry for that road then."""
import pickle

import numpy as np
import pytest

import maskutil as M
from gym_TD.masks import reference_masks
from oracle import td_oracle as O

L = 10
NC = L * L
STEPS = 300
CHECK_AT = range(7, STEPS, 50)


def _clone(env):
    return pickle.loads(pickle.dumps(env, pickle.HIGHEST_PROTOCOL))


def _masks(env, mode, multi):
    return reference_masks(M.oracle_state(env), env.L, env.cfg, env.hp, mode, multi, cap=False)


def _brute_def(env, multi):
    """(mask, code) of every defender action by stepping copies of env."""
    blob = pickle.dumps(env, pickle.HIGHEST_PROTOCOL)
    mask = np.zeros(6 * NC, dtype=np.uint8)
    code = np.zeros(6 * NC, dtype=np.uint8)
    b = None
    for k in range(6 * NC):
        e = pickle.loads(blob)
        _, _, _, info = e.step(M.def_action(k, L, multi))
        real = info["RealAction"]
        mask[k] = (real.reshape(-1)[k] == 1) if multi else (real == k)
        # the operation itself, the cool-down aside (a failed one leaves the board as it was)
        if b is None:
            b = pickle.loads(blob)._board
        op, cell = divmod(k, NC)
        loc = [cell // L, cell % L]
        ok = b.tower_build(op, loc) if op < 4 else b.tower_lvup(loc) if op == 4 else b.tower_destruct(loc)
        code[k] = b.fail_code
        if ok:
            b = None
    return mask, code


@pytest.fixture(scope="module")
def rich_runs():
    """Discrete TD-def, rich config, seeds 0, 2, 3, 4 (seed 1's first road draw fails):
    300 steps of the mask policy each; counts of the operation classes taken, the codes seen,
    the cool-down-blocked steps, and what went wrong (a brute-force mismatch at CHECK_AT, a
    chosen action the step did not execute)."""
    cfg = M.config(M.RICH)
    seeds, envs = M.ok_seeds(L, 4, 0, O.MODE_DEF, cfg=cfg)
    out = {"seeds": seeds, "ops": np.zeros(6, dtype=int), "codes": set(), "blocked": 0, "steps": 0, "checks": 0,
           "bad": []}
    for s, env in zip(seeds, envs):
        rng = np.random.RandomState(1000 + s)
        for k in range(STEPS):
            mask, code, _ = _masks(env, "def", False)
            if k in CHECK_AT:
                bm, bc = _brute_def(env, False)
                out["checks"] += 1
                if not (np.array_equal(mask[:-1], bm) and np.array_equal(code[:-1], bc) and mask[-1] == 1 and
                        code[-1] == 0):
                    out["bad"].append(("brute", s, k))
            out["codes"].update(int(c) for c in np.unique(code))
            out["blocked"] += int(env.defender_cd > 1)
            out["steps"] += 1
            a = M.pick_def(rng, mask, NC)
            _, _, done, info = env.step(M.def_action(a, L, False))
            if a >= 0:
                out["ops"][a // NC] += 1
                if info["RealAction"] != a or info["FailCode"] != 0:
                    out["bad"].append(("chosen", s, k, a))
            if done:
                M.reset_ok(env)
    return out


def test_rich_seeds_are_the_issue_seeds(rich_runs):
    assert rich_runs["seeds"] == [0, 2, 3, 4]


def test_defender_discrete_equals_brute_force(rich_runs):
    assert rich_runs["checks"] == 4 * len(CHECK_AT)
    assert not rich_runs["bad"], rich_runs["bad"][:5]


def test_rich_run_reaches_every_case(rich_runs):
    # so the comparison cannot pass on an empty case
    assert (rich_runs["ops"] > 0).all(), rich_runs["ops"]  # build x 4 types, level-up, destruct
    assert {0, 1, 2, 3, 4} <= rich_runs["codes"], rich_runs["codes"]
    assert 0 < rich_runs["blocked"] < rich_runs["steps"]


def test_defender_multi_equals_brute_force():
    cfg = M.config(M.RICH)
    seeds, envs = M.ok_seeds(L, 2, 0, O.MODE_DEF, multi=True, cfg=cfg)
    checks = 0
    for s, env in zip(seeds, envs):
        rng = np.random.RandomState(1000 + s)
        for k in range(120):
            mask, code, _ = _masks(env, "def", True)
            assert mask.shape == code.shape == (6, L, L)
            if k in (7, 57, 107):
                bm, bc = _brute_def(env, True)
                assert np.array_equal(mask.reshape(-1), bm), (s, k)
                assert np.array_equal(code.reshape(-1), bc), (s, k)
                checks += 1
            a = M.pick_def(rng, mask, NC)
            _, _, done, info = env.step(M.def_action(a, L, True))
            if a >= 0:
                assert info["RealAction"].reshape(-1)[a] == 1 and info["RealAction"].sum() == 1, (s, k, a)
            if done:
                M.reset_ok(env)
    assert checks == 6


def _summoned(info, rt):
    fc, real = info["FailCode"], info["RealAction"]
    return len(fc) > rt[0] and fc[rt[0]] == 0 and int(real[rt[0]][0]) == rt[1]


@pytest.mark.parametrize("max_steps", [1200, 40])
def test_attacker_equals_brute_force(max_steps):
    """TD-atk, cluster [t, 4, 4, ...] on one road.  max_steps = 40: the level switch at
    progress 0.75 (step 30) decides entries, since level 1 costs 7 more."""
    cfg, hp = M.config(M.ATK), M.hyper(max_episode_steps=max_steps)
    seeds, envs = M.ok_seeds(L, 3, 0, O.MODE_ATK, cfg=cfg, hp=hp)
    seen = {"blocked": 0, "no_road": 0, "poor": 0, "lv_decides": 0, "taken": 0}
    for s, env in zip(seeds, envs):
        rng = np.random.RandomState(1000 + s)
        for k in range(120):
            _, _, mask = _masks(env, "atk", False)
            assert mask.shape == (3, 5) and (mask[:, 4] == 1).all()
            for road in range(3):
                for t in range(4):
                    e = _clone(env)
                    _, _, _, info = e.step(atk_act=M.atk_action((road, t)))
                    assert mask[road, t] == _summoned(info, (road, t)), (s, k, road, t)
            b = env._board
            seen["blocked"] += int(env.attacker_cd > 1)
            seen["no_road"] += int(env.num_roads < 3)
            seen["poor"] += int(mask[0, :4].min() == 0 and env.attacker_cd <= 1)
            lv = int(b.steps / hp.max_episode_steps >= cfg.enemy_upgrade_at)
            seen["lv_decides"] += int(lv == 1 and env.attacker_cd <= 1 and any(
                cfg.enemy_cost[t][0] <= b.cost_atk < cfg.enemy_cost[t][1] for t in range(4)))
            rt = M.pick_atk(rng, mask)
            _, _, done, info = env.step(atk_act=M.atk_action(rt))
            if rt is not None:
                assert _summoned(info, rt), (s, k, rt)
                seen["taken"] += 1
            if done:
                M.reset_ok(env)
    assert seen["blocked"] and seen["no_road"] and seen["poor"] and seen["taken"], seen
    if max_steps == 40:
        assert seen["lv_decides"], seen


def test_capacity_rule_is_optional():
    """cap=True adds the device's two rules (code 6 at 32 towers, no summon at 128 enemies)."""
    cfg, hp = M.config(M.CAP), M.hyper()
    st = {"steps": 5, "cost_def": 500.0, "cost_atk": 500.0, "attacker_cd": 0, "defender_cd": 0, "num_roads": 2,
          "towers": [(0, 0, r, c, 0.0) for r in range(4) for c in range(8)], "enemies": [None] * 128,
          "map6": [1 if (i // L < 4 and i % L < 8) else 0 for i in range(NC)]}
    m0, c0, a0 = reference_masks(st, L, cfg, hp, "2p", False, cap=False)
    m1, c1, a1 = reference_masks(st, L, cfg, hp, "2p", False, cap=True)
    free = np.asarray(st["map6"]) == 0
    assert (c0[:4 * NC].reshape(4, NC)[:, free] == 0).all() and (m0[:4 * NC].reshape(4, NC)[:, free] == 1).all()
    assert (c1[:4 * NC].reshape(4, NC)[:, free] == 6).all() and (m1[:4 * NC].reshape(4, NC)[:, free] == 0).all()
    assert np.array_equal(c0[4 * NC:], c1[4 * NC:]) and np.array_equal(m0[4 * NC:], m1[4 * NC:])
    assert (a0[:2, :4] == 1).all() and (a0[2, :4] == 0).all() and (a1[:, :4] == 0).all() and (a1[:, 4] == 1).all()
