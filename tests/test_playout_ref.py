"""The rule of td_playout on the CPU (no GPU): gym_TD.sampling.reference_playout on the Python
oracle for the cases the GPU anchor uses (tests/playoutref.py), split invariance, and the event
ledger with its floors -- each met on the CPU alone, so that what the GPU anchor compares is known
to contain every kind of sub-step."""
import copy

import numpy as np
import pytest

import maskutil as M
import playoutref as PR
from gym_TD import sampling as S
from gym_TD.masks import reference_masks

FLOOR = 20


@pytest.fixture(scope="module")
def anchor():
    led = PR.new_ledger()
    runs = {c["name"]: PR.run_case(c, led) for c in PR.ANCHOR_CASES}
    return runs, led


def test_anchor_cases_run(anchor):
    """Every anchor case: the results' shape, the rewards added left to right, a board that stops
    at its episode's end, first actions in the sampler's formats."""
    runs, _ = anchor
    assert set(runs) == {"def", "atk", "2p"}
    for case in PR.ANCHOR_CASES:
        ref = runs[case["name"]]
        assert len(ref["rounds"]) == case["rounds"]
        for (k, _), rnd in zip(PR.round_plan(case), ref["rounds"]):
            assert len(rnd) == case["n"] and 1 <= k <= case["k"]
            for res in rnd:
                assert 1 <= res["steps_run"] <= k and len(res["events"]) == res["steps_run"]
                assert res["done"] or res["steps_run"] == k
                assert isinstance(res["reward"], float)
                assert (res["first_def"] is None) == (case["mode"] == "atk")
                assert (res["first_atk"] is None) == (case["mode"] == "def")
                if res["first_atk"] is not None:
                    assert res["first_atk"].shape == (3, 8) and res["first_atk"].dtype == np.int64


def test_sampled_actions_are_executed():
    """Along a playout the env executes what was sampled: FailCode 0 in every sub-step (TD-def)."""
    cfg, hp = PR.anchor_config()
    (seed,), (env,) = M.ok_seeds(10, 1, 500, PR.MODES["def"], cfg=cfg, hp=hp)
    acted = 0
    for r in range(12):
        twin = copy.deepcopy(env)
        res = S.reference_playout(env, M.oracle_state, 10, cfg, hp, "def", 3, 5 * r, 0, 5, 0.3, 0.3, cap=False)
        for j, ev in enumerate(res["events"]):  # the same sub-steps by hand on the copy
            a = 600 if ev["def"] is None else ev["def"]
            _, _, _, info = twin.step(def_act=a)
            assert info["RealAction"] == a and (a == 600 or info["FailCode"] == 0), (r, j, a, info)
            acted += int(a != 600)
        if res["done"]:
            M.reset_ok(env)
    assert acted > 5


@pytest.mark.parametrize("mode", ["def", "atk", "2p"])
def test_split_invariance(mode):
    """k1 + k2 sub-steps from ticket t equal k1 from t, then k2 from t + k1: the same env state and
    counts, the same first actions, and the reward to rounding (two partial sums)."""
    cfg, hp = PR.anchor_config()
    hp.max_episode_steps = 60
    seeds, envs = M.ok_seeds(10, 4, 500, PR.MODES[mode], cfg=cfg, hp=hp)
    for b, env in enumerate(envs):
        for k1, k2 in ((3, 4), (1, 9), (6, 1)):
            whole = copy.deepcopy(env)
            one = S.reference_playout(whole, M.oracle_state, 10, cfg, hp, mode, 9, 40, b, k1 + k2, 0.3, 0.3)
            p1 = S.reference_playout(env, M.oracle_state, 10, cfg, hp, mode, 9, 40, b, k1, 0.3, 0.3)
            run, rew, done = p1["steps_run"], p1["reward"], p1["done"]
            if not done:
                p2 = S.reference_playout(env, M.oracle_state, 10, cfg, hp, mode, 9, 40 + k1, b, k2, 0.3, 0.3)
                run, rew, done = run + p2["steps_run"], rew + p2["reward"], p2["done"]
                assert one["events"] == p1["events"] + p2["events"]
            assert (one["steps_run"], one["done"]) == (run, done), (b, k1, k2)
            assert abs(one["reward"] - rew) <= 1e-9 * max(1.0, abs(rew))
            assert str(M.oracle_state(whole)) == str(M.oracle_state(env)), (b, k1, k2)
            assert np.array_equal(one["first_def"], p1["first_def"]) and np.array_equal(one["first_atk"], p1["first_atk"])
            if done:
                M.reset_ok(env)


def test_ticket_wraps_mod_2_64():
    """Sub-step 1 of a playout from ticket 2^64 - 1 draws at ticket 0."""
    cfg, hp = PR.anchor_config()
    (seed,), (env,) = M.ok_seeds(10, 1, 500, PR.MODES["2p"], cfg=cfg, hp=hp)
    twin = copy.deepcopy(env)
    res = S.reference_playout(env, M.oracle_state, 10, cfg, hp, "2p", 9, S.M64, 0, 3)
    for j, ticket in enumerate((S.M64, 0, 1)):
        dm, _, am = reference_masks(M.oracle_state(twin), 10, cfg, hp, "2p", False)
        d, a, _, _ = S.reference_sample(dm, am, 9, ticket, 0, 0, 0, 10, False)
        ev = res["events"][j]
        assert ev["def"] == (None if d == 600 else d), j
        roads = np.flatnonzero(a[:, 0] != 4)
        assert ev["atk"] == ((int(roads[0]), int(a[roads[0], 0])) if len(roads) else None), j
        twin.step(def_act=d, atk_act=a)


def test_event_ledger_floors(anchor):
    """Over the anchor cases together, at least 20 each of: sampled builds, level-ups, destructs,
    summons, idle draws that fired, sub-steps with nothing legal; episodes ending inside a playout
    at no fewer than 5 distinct sub-step positions from each of the two causes (base LP and the
    step limit)."""
    _, led = anchor
    print("ledger:", {k: (v if not isinstance(v, dict) else {a: sorted(b) for a, b in v.items()}) for k, v in led.items()})
    for name in ("build", "lvup", "destruct", "summon", "idle_fired", "nothing_legal"):
        assert led[name] >= FLOOR, (name, led[name])
    ends = led["ends"]
    assert len(ends["base"]) >= 5 and len(ends["limit"]) >= 5, ends


@pytest.mark.parametrize("mode,regime,seed", PR.CROWD_CASES)
def test_crowd_cases_reach_their_floors(mode, regime, seed):
    """swarm: some board above 16 live enemies; fortress: some board at 32 towers, where build
    code 6 removes the build candidates (reference_masks with the device's capacity rule)."""
    cfg, hp = PR.crowd_config(regime, seed)
    seeds, envs = M.ok_seeds(10, 4, 500, PR.MODES[mode], cfg=cfg, hp=hp)
    led = PR.new_ledger()
    capped = 0
    for r in range(PR.CROWD_ROUNDS):
        PR.play(envs, seeds, 10, cfg, hp, mode, 16, 16 * r, 0, led)
        for env in envs:
            st = M.oracle_state(env)
            if len(st["towers"]) == 32 and mode != "atk":
                _, code, _ = reference_masks(st, 10, cfg, hp, mode, False)
                capped += int((code[:400] == 6).any())
    print("crowd %s %s: enemies %d towers %d capped %d" % (mode, regime, led["top_enemies"], led["top_towers"], capped))
    if regime == "swarm":
        assert led["top_enemies"] > 16
    else:
        assert led["top_towers"] == 32 and capped > 0
