"""The twelve fuzzed-config cases of tests/cfgspace.py on the CPU: the Python oracle against the C
restatement at every step of every board (reward bits, state digest, observation bytes), and
the reach of the cases -- what the oracle did under them, counted by cfgspace.Ledger.  The GPU
test (tests/test_gpu_config_space.py) runs the same cases; this file is where a difference
between the device and the oracle is first narrowed down (reference fixtures: the ``cfg_*``
goldens; oracle against oracle: here).

The C binding draws its own roads, so it cannot take the 7x7 case (caller-made roads): that case
runs on the Python oracle alone and still counts into the ledger."""
import numpy as np
import pytest

import cfgspace as S
from oracle import canon
from oracle import td_cpu as C

_RESULTS = {}


def _run(case):
    """The case on both oracles: (its ledger, the first difference or None, boards finished)."""
    if case.name in _RESULTS:
        return _RESULTS[case.name]
    cfg = case.cfg()
    seeds, envs = S.make_envs(case, cfg)
    cenvs = None
    if case.L != 7:
        cenvs = [C.Env(case.L, case.mode, case.difficulty, s, s, cfg, multi=case.multi, road_attempts=1000) for s in seeds]
    led, bad = S.Ledger(), None
    rng = np.random.RandomState(case.seed)
    try:
        with S.recording(led):
            for k in range(case.steps):
                da, aa = S.draw_actions(case, rng, envs)
                for b, o in enumerate(envs):
                    if o._board.done():
                        continue
                    d, a = S.act_of(case, da, aa, b)
                    wo, wr, wd, _ = o.step(d, a)
                    if cenvs is None or bad is not None:
                        continue
                    ob, r, dn = cenvs[b].step(d, a)
                    if canon.fhex(r) != canon.fhex(wr) or dn != wd:
                        bad = (k, b, "reward/done", canon.fhex(r), canon.fhex(wr), dn, wd)
                    elif canon.digest(cenvs[b].state_bytes()) != canon.state_digest(canon.oracle_state(o)):
                        bad = (k, b, "state")
                    elif not np.array_equal(ob, S.pad_obs(wo)):
                        bad = (k, b, "obs", np.argwhere(ob != S.pad_obs(wo))[:5].tolist())
    finally:
        for c in cenvs or ():
            c.close()
    assert all(getattr(o, "refused", [0, 0]) == [0, 0] for o in envs), case.name
    done = sum(o._board.done() for o in envs)
    _RESULTS[case.name] = (led, bad, done)
    return _RESULTS[case.name]


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_oracles_agree_on_fuzzed_configs(name):
    """Reward bits, done, state digest and all observation bytes of every board at every step;
    the lists stay within the device's capacities (128 enemies, 32 towers), so the GPU run of the
    case raises no flag."""
    led, bad, _ = _run(S.CASE[name])
    assert bad is None, bad
    assert led.max_enemies <= S.ENEMY_CAP and led.max_towers <= S.TOWER_CAP, (led.max_enemies, led.max_towers)


def test_draw_is_deterministic_and_json_clean():
    """draw() depends on (seed, regime) alone, its values survive JSON (the fixtures carry them)
    and every double-typed field has a full mantissa unless an edge was planted."""
    import json
    for regime in S.REGIMES:
        a, b = S.draw(5, regime), S.draw(5, regime)
        assert a == b and json.loads(json.dumps(a)) == a
        assert a != S.draw(6, regime)
        assert all(isinstance(a[k], int) for k in ("frozen_time", "tower_distance", "attacker_action_interval",
                                                   "defender_action_interval", "base_LP", "max_tower_lv"))
        vals = [v for name in S.TABLES for row in a[name] for v in row]
        full = [v for v in vals if v != 0.0 and float(np.float32(v)) != v]
        assert len(full) >= len(vals) - 12, (regime, len(full), len(vals))
    edges = dict(range0=0, range_big=0, splash0=0, floor=0, equal=0, ratio0=0, ratio_big=0, ret_big=0, fast=0,
                 up0=0, up_big=0, rate0=0)
    for seed in range(200):  # every planted edge occurs
        ov = S.draw(seed, S.REGIMES[seed % 4])
        atk = [v for r in ov["tower_attack"] for v in r]
        dfs = [v for r in ov["enemy_defense"] for v in r]
        edges["range0"] += any(v == 0.0 for r in ov["tower_range"] for v in r)
        edges["range_big"] += any(v >= 32 for r in ov["tower_range"] for v in r)
        edges["splash0"] += any(v == 0.0 for v in ov["tower_splash_range"][2] + ov["tower_splash_range"][3])
        edges["floor"] += max(dfs) > max(atk)
        edges["equal"] += any(v in atk for v in dfs)
        edges["ratio0"] += ov["frozen_ratio"] == 0.0
        edges["ratio_big"] += ov["frozen_ratio"] > 1
        edges["ret_big"] += ov["tower_destruct_return"] > 1
        edges["fast"] += any(1 <= v <= 2.9 for r in ov["enemy_speed"] for v in r)
        edges["up0"] += ov["enemy_upgrade_at"] == 0.0
        edges["up_big"] += ov["enemy_upgrade_at"] > 1
        edges["rate0"] += any(ov[k] == 0.0 for k in ("attacker_cost_init_rate", "attacker_cost_final_rate",
                                                      "defender_cost_rate"))
    assert all(v >= 5 for v in edges.values()), edges


def test_cases_reach_the_rule_arithmetic():
    """Over the twelve cases together every event of cfgspace.Ledger occurs at least 20 times.
    Observed: shots that hit, by tower type, level 0 / level 1: arrow 5712 / 496, magic 194 / 100,
    bomb 247 / 189, freezer 1487 / 210; floored 566, bomb_multi 99, multi_kill 67, frozen_hits
    1697, slowed_marches 2059, long_marches 924, multi_leak_steps 83, leaks_at_zero 66,
    over16_steps 4037, eq16_steps 166, eq17_steps 253, shared_cell_steps 5606, capped_destructs
    6514, def_at_max_steps 1226, atk_at_max_steps 587, lv1_summons 1429, lv0_refused_upgrades 883,
    cooldown_over15 2089."""
    total = S.Ledger()
    for case in S.CASES:
        led = _run(case)[0]
        for k, v in led.hits.items():
            total.hits[k] += v
        for k in S._EVENTS:
            setattr(total, k, getattr(total, k) + getattr(led, k))
    print(total.as_dict())
    assert not total.short(), total.short()
