"""Fuzzed game configs: the generator, the twelve cases built on it and the oracle-side event
ledger.  Shared by tests/golden/gen_golden.py (the ``cfg_*`` fixtures), tests/test_config_space_ref.py
(CPU: the two oracles against each other, and the reach of the cases) and
tests/test_gpu_config_space.py (the device against the oracle).  Not a test module.

Every other parameter set of the suite is made of short decimals and small integers, under which
nearly every f64 operation of the rules is exact.  ``draw(seed, regime)`` gives every double-typed
field of the config a value with a full mantissa -- a default times a random factor -- draws the
integer-typed fields from small sets that hold their edges, and plants the edge values of the rule
arithmetic (a range of 0, a defense equal to an attack, a frozen_ratio above 1, ...) with fixed
probabilities.  A regime biases the draw towards a kind of game; it never fixes a value."""
import contextlib

import numpy as np

from oracle import td_oracle as O

REGIMES = ("balanced", "swarm", "fortress", "sprint")
TABLES = ("enemy_LP", "enemy_speed", "enemy_defense", "enemy_cost", "tower_attack", "tower_range",
          "tower_splash_range", "tower_cost", "tower_attack_interval")
ENEMY_CAP, TOWER_CAP = 128, 32  # the device's list capacities (include/tdstep.h td_board_flag)

# per regime: (field, factor) applied to the defaults before the jitter
_BIAS = {
    "balanced": {},
    # cheap, slow, sturdy enemies and a rich attacker: crowds above 16, leaks by the cluster
    "swarm": dict(enemy_cost=0.22, enemy_speed=0.5, enemy_LP=2.2, enemy_defense=1.3, attacker_cost_init_rate=3.0,
                  attacker_cost_final_rate=3.0, defender_cost_rate=1.5, max_cost=0.35),
    # rich defender, cheap upgrades: level-1 towers fire, cost_def sits at max_cost
    "fortress": dict(defender_init_cost=5.0, defender_cost_rate=9.0, tower_cost_lv1=0.3, max_cost=0.7,
                     tower_attack=1.5, attacker_cost_init_rate=2.0, attacker_cost_final_rate=2.0),
    # speeds above 1 and short episodes
    "sprint": dict(enemy_speed=9.0, enemy_LP=1.5, attacker_cost_init_rate=2.0, defender_cost_rate=2.0),
}
_INT_SETS = dict(frozen_time=(0, 1, 2, 3, 7), tower_distance=(0, 1, 2, 3, 5),
                 attacker_action_interval=(1, 2, 3, 17), defender_action_interval=(1, 2, 3, 17),
                 base_LP=(1, 2, 5), max_tower_lv=(0, 1))
# the regimes' weights over those sets (balanced: uniform)
_INT_W = {
    "swarm": dict(base_LP=(.2, .4, .4), attacker_action_interval=(.25, .2, .2, .35)),
    "fortress": dict(tower_distance=(.05, .15, .35, .3, .15), defender_action_interval=(.6, .25, .1, .05),
                     max_tower_lv=(.25, .75)),
    "sprint": dict(base_LP=(.45, .45, .1)),
}
PLANT = 0.3  # probability of each planted edge value


def draw(seed, regime="balanced"):
    """The overrides (every field of the config, JSON-clean: floats, ints, lists) of draw
    ``seed`` in ``regime``; deterministic from numpy.random.RandomState(seed)."""
    assert regime in REGIMES, regime
    rng = np.random.RandomState(seed)
    d, bias = O.Config(), _BIAS[regime]
    u = lambda lo, hi: float(rng.uniform(lo, hi))
    coin = lambda p=PLANT: bool(rng.random_sample() < p)
    slot = lambda: (int(rng.randint(4)), int(rng.randint(2)))
    ov = {}
    for name in TABLES:
        f = bias.get(name, 1.0)
        ov[name] = [[float(v) * f * u(0.75, 1.3) for v in row] for row in getattr(d, name)]
    # defaults of 0 have no mantissa to jitter: drawn, not multiplied
    ov["enemy_defense"][0] = [u(0.0, 70.0), u(0.0, 90.0)]
    for t in (0, 1, 3):
        ov["tower_splash_range"][t] = [u(0.0, 1.7), u(0.0, 2.2)]  # (arrow / magic towers never read theirs)
    for t in range(4):
        ov["tower_cost"][t][1] *= bias.get("tower_cost_lv1", 1.0)
    for name in ("tower_destruct_return", "frozen_ratio", "defender_init_cost", "max_cost", "reward_kill",
                 "penalty_leak", "reward_time", "attacker_cost_init_rate", "attacker_cost_final_rate",
                 "defender_cost_rate", "enemy_upgrade_at"):
        ov[name] = float(getattr(d, name)) * bias.get(name, 1.0) * u(0.75, 1.3)
    ov["attacker_init_cost"] = u(0.0, 25.0) * bias.get("attacker_init_cost", 1.0)
    ov["enemy_upgrade_at"] = u(0.05, 0.5)  # level-1 enemies inside runs of 120-400 steps of 1200
    for name, values in _INT_SETS.items():
        ov[name] = int(values[rng.choice(len(values), p=_INT_W.get(regime, {}).get(name))])
    # ---- planted edges
    if coin():
        ov["tower_range"][slot()[0]][0] = 0.0
    if coin():
        t, l = slot()
        ov["tower_range"][t][l] = u(1.0, 3.0)
    if coin():
        t, l = slot()
        ov["tower_range"][t][l] = 32.0 + u(0.0, 9.0)  # >= L for every map size
    if coin():
        ov["tower_splash_range"][2][int(rng.randint(2))] = 0.0
    if coin():
        ov["tower_splash_range"][3][int(rng.randint(2))] = 0.0
    if coin(0.5):  # a defense above every attack: each arrow / bomb hit on it is the 5 % floor
        t, l = slot()
        ov["enemy_defense"][t][l] = max(max(r) for r in ov["tower_attack"]) * u(1.01, 1.5)
    if coin(0.5):  # and one exactly equal to an attack: atk - def = 0
        t, l = slot()
        ov["enemy_defense"][t][l] = ov["tower_attack"][int(rng.choice((0, 2)))][int(rng.randint(2))]
    if coin():
        ov["frozen_ratio"] = 0.0
    elif coin():
        ov["frozen_ratio"] = u(1.0, 1.8)
    if coin():
        ov["tower_destruct_return"] = u(1.0, 2.5)
    fast = regime == "sprint"
    for t in range(4):
        for l in range(2):
            if fast or coin(0.15):
                ov["enemy_speed"][t][l] = u(1.0, 2.9)
    if coin(0.15):
        ov["enemy_upgrade_at"] = 0.0
    elif coin(0.15):
        ov["enemy_upgrade_at"] = u(1.0, 1.5)
    if coin(0.2):
        ov[("attacker_cost_init_rate", "attacker_cost_final_rate", "defender_cost_rate")[int(rng.randint(3))]] = 0.0
    return ov


def config(seed, regime):
    return O.Config(**draw(seed, regime))


def pad_obs(obs):
    """The device's observation always has 45 planes.  With max_tower_lv = 0 the reference's has
    44 (TDBoard.py:146-154: one tower-level plane); the device's are those with an all-zero
    plane 16 in between, so that every other channel keeps its index."""
    if obs.shape[0] == 45:
        return obs
    assert obs.shape[0] == 44
    return np.concatenate([obs[:16], np.zeros_like(obs[:1]), obs[16:]])


# --------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------
# Roads of the 7x7 case (create_road_v2 cannot draw a 7x7 map): even boards the straight one,
# odd boards the two that merge -- the maps of maskutil.hand_layouts_7.
_TOP7 = [(1, c) for c in range(7)]
ROADS7 = ([[(3, c) for c in range(7)]],
          [_TOP7, [(5, 0), (5, 1), (5, 2), (5, 3), (4, 3), (3, 3), (2, 3)] + _TOP7[3:]])


class Case(object):
    """One (seed, regime, mode) case: B boards of L x L from seed0, ``steps`` steps.
    ``kernels``: the step kernels the device runs it on; ``variants``: the further device runs
    ("f16", "skip3", "partial", "switch").  ``reach``: the least share of its B x steps board-steps
    that the oracle steps before the boards finish (measured: 0.91-1.0 where nothing is said; the
    sprint cases, whose episodes are short by design, 0.32-0.44; the 20x20 case 0.78)."""

    def __init__(self, name, seed, regime, mode, multi, difficulty, L=10, B=16, steps=150, small=None, variants=(),
                 reach=0.85):
        self.reach = reach
        self.name, self.seed, self.regime, self.mode, self.multi = name, seed, regime, mode, multi
        self.difficulty, self.L, self.B, self.steps = difficulty, L, B, steps
        self.kernels = ("large",) + ((small,) if small else ())
        self.variants = tuple(variants)
        self.seed0 = 9000 + 100 * seed

    def cfg(self):
        return config(self.seed, self.regime)

    def hyper(self):
        return O.Hyper(allow_multiple_actions=self.multi)


CASES = [
    Case("bal-def", 16, "balanced", "def", False, 1, small="small", variants=("f16", "switch")),
    Case("swarm-def", 12, "swarm", "def", False, 1, small="small2", variants=("f16", "skip3")),
    Case("fort-def", 17, "fortress", "def", False, 1, small="small", variants=("f16", "partial")),
    Case("sprint-def", 29, "sprint", "def", False, 1, small="small2", variants=("f16", "skip3"), reach=0.3),
    Case("bal-atk2", 16, "balanced", "atk", False, 2, small="small", variants=("skip3",)),
    Case("swarm-2p", 6, "swarm", "2p", False, 1, small="small2", variants=("skip3",)),
    Case("fort-2pmulti", 12, "fortress", "2p", True, 1, steps=120, small="small", variants=("partial", "switch")),
    Case("sprint-atk1", 29, "sprint", "atk", False, 1, small="small2", reach=0.3),
    Case("swarm-def0", 20, "swarm", "def", False, 0, small="small", variants=("partial",)),
    Case("fort-atk1", 32, "fortress", "atk", False, 1, small="small2", variants=("partial",)),
    Case("sprint-def7", 3, "sprint", "def", False, 1, L=7, steps=120, reach=0.3),
    Case("bal-2pmulti20", 27, "balanced", "2p", True, 1, L=20, B=6, steps=120, reach=0.7),
]
CASE = {c.name: c for c in CASES}
SWITCH_AT, SWITCH_TO = 50, (101, "swarm")  # the "switch" variant: set_config(draw(*SWITCH_TO)) before step 50


def switch_overrides(case):
    """The second config of the "switch" variant.  It keeps the first one's max_tower_lv (a
    level-1 tower under max_tower_lv = 0 has no plane in the reference's observation), and its
    tower_distance is below the first one's where that is above 0: td_set_config refuses a
    tower_distance that grows while towers stand (include/tdstep.h), and a smaller one leaves the
    destructed towers' outer cells counted, as in the reference.  base_LP / max_cost reach only
    boards reset afterwards, as in the reference."""
    ov, first = draw(*SWITCH_TO), draw(case.seed, case.regime)
    ov["max_tower_lv"] = first["max_tower_lv"]
    ov["tower_distance"] = min(ov["tower_distance"], max(first["tower_distance"] - 1, 0))
    return ov


def make_envs(case, cfg=None, env_cls=None):
    """(seeds, oracle envs) of a case; at L = 7 the envs run on ROADS7 (handmaps.HandEnv)."""
    import handmaps
    import maskutil
    cfg = cfg or case.cfg()
    if case.L == 7:
        envs = [handmaps.HandEnv(ROADS7[b % 2], 7, handmaps.MODES[case.mode], case.difficulty, case.seed0 + b, cfg,
                                 case.hyper()) for b in range(case.B)]
        return [case.seed0 + b for b in range(case.B)], envs
    return maskutil.ok_seeds(case.L, case.B, case.seed0, handmaps.MODES[case.mode], case.multi, case.difficulty,
                             cfg, case.hyper())


def draw_actions(case, rng, envs):
    """One step's caller actions for all boards (finished ones included, so that the stream does
    not depend on who finished): (def [B] / [B, 6, L, L] or None, atk [B, 3, 8] or None)."""
    from oracle import policies
    L, da, aa = case.L, None, None
    if case.mode != "atk":
        if case.multi:
            da = np.stack([policies.multi_def(rng, L) for _ in envs]).astype(np.int64)
        else:
            da = np.array([policies.discrete_def(rng, L, o._board.map[0], 0.8) for o in envs], dtype=np.int64)
    if case.mode != "def":
        aa = np.stack([policies.atk(rng) for _ in envs]).astype(np.int64)
    return da, aa


def act_of(case, da, aa, b):
    d = None if da is None else (da[b] if case.multi else int(da[b]))
    return d, (None if aa is None else aa[b])


# --------------------------------------------------------------------------
# the event ledger
# --------------------------------------------------------------------------
LEDGER_MIN = 20
_EVENTS = ("floored", "bomb_multi", "multi_kill", "frozen_hits", "slowed_marches", "long_marches", "multi_leak_steps",
           "leaks_at_zero", "over16_steps", "eq16_steps", "eq17_steps", "shared_cell_steps", "capped_destructs",
           "def_at_max_steps", "atk_at_max_steps", "lv1_summons", "lv0_refused_upgrades", "cooldown_over15")


class Ledger(object):
    """What the oracle did, over the board-steps counted:

    hits[(type, lv)]      shots that found a target, per tower type and level
    floored               arrow / bomb damage raised to 5 % of the attack (TDElements.py:23-24)
    bomb_multi            bomb shots that damaged at least 2 enemies
    multi_kill            shots that left at least 2 enemies at LP 0
    frozen_hits           freezer shots;  slowed_marches: marches made at speed * frozen_ratio
    long_marches          marches of at least 2 cells in one step
    multi_leak_steps      board-steps with at least 2 leaks
    leaks_at_zero         leaks onto a base already at 0 (no penalty_leak, TDBoard.py:331-334)
    over16 / eq16 / eq17_steps   board-steps entered with > 16 / 16 / 17 live enemies
    shared_cell_steps     board-steps that leave >= 3 enemies of one type in one cell
    capped_destructs      destructs whose return was cut by max_cost
    def_at_max / atk_at_max_steps   board-steps that leave cost_def / cost_atk == max_cost
    lv1_summons           level-1 enemies summoned
    lv0_refused_upgrades  upgrades refused with FAIL_LVMAX under max_tower_lv = 0
    cooldown_over15       env steps that leave a cool-down above 15 (the 4-bit output saturates)
    max_enemies / max_towers   the longest lists seen"""

    def __init__(self):
        self.hits = {(t, l): 0 for t in range(4) for l in range(2)}
        for k in _EVENTS:
            setattr(self, k, 0)
        self.max_enemies = self.max_towers = 0

    def as_dict(self):
        d = {"hits_t%d_lv%d" % k: v for k, v in sorted(self.hits.items())}
        d.update((k, getattr(self, k)) for k in _EVENTS)
        return d

    def short(self):
        """Every event that the cases together must reach LEDGER_MIN times and did not."""
        return {k: v for k, v in self.as_dict().items() if v < LEDGER_MIN}


@contextlib.contextmanager
def recording(led):
    """Inside the block the oracle's ``_fire``, ``Enemy.hit``, ``Board.step``, the board
    operations and ``Env.step`` report to ``led``.  The wrappers only read and call the unchanged
    originals: a recorded trajectory is the trajectory."""
    fire0, hit0, step0, env_step0 = O._fire, O.Enemy.hit, O.Board.step, O.Env.step
    summon0, lvup0, destruct0 = O.Board.summon_cluster, O.Board.tower_lvup, O.Board.tower_destruct
    frozen = set()  # ids of the enemies frozen in the board-step under way

    def fire(tw, enemies, cfg):
        tgt = next((e for e in enemies if O._cheb(e.loc, tw.loc) <= tw.rge), None)
        if tgt is not None:
            led.hits[(tw.type, tw.lv)] += 1
            if tw.type >= 2:
                near = [e for e in enemies if O._cheb(tgt.loc, e.loc) <= tw.dmgrge]
                if tw.type == 2:
                    led.bomb_multi += len(near) >= 2
                else:
                    led.frozen_hits += 1
                    # _fire freezes the first enemy, in the order of ``enemies``, within the splash of the
                    # target (its loop breaks there, TDElements.py:118-132); ``near`` is in that order
                    frozen.add(id(near[0]))
        out = fire0(tw, enemies, cfg)
        led.multi_kill += len(out) >= 2
        return out

    def hit(e, atk, magic=False):
        led.floored += (not magic) and max(atk - e.defense, 0) < atk * .05
        return hit0(e, atk, magic)

    def step(board):
        before = list(board.enemies)
        n = len(before)
        led.max_enemies, led.max_towers = max(led.max_enemies, n), max(led.max_towers, len(board.towers))
        led.over16_steps += n > 16
        led.eq16_steps += n == 16
        led.eq17_steps += n == 17
        was = {id(e): (e.slowdown, e.dist) for e in before}
        base = board.base_LP
        frozen.clear()
        reward = step0(board)
        left = set(id(e) for e in board.enemies)
        leaks = 0
        for e in before:
            if not e.LP > 0:
                continue  # killed: it did not march
            slow, dist = was[id(e)]
            led.slowed_marches += (board.cfg.frozen_time if id(e) in frozen else slow) > 0
            led.long_marches += dist - e.dist >= 2
            leaks += id(e) not in left
        led.multi_leak_steps += leaks >= 2
        led.leaks_at_zero += max(0, leaks - base)
        groups = {}
        for e in board.enemies:
            g = (e.type, e.loc[0], e.loc[1])
            groups[g] = groups.get(g, 0) + 1
        led.shared_cell_steps += any(v >= 3 for v in groups.values())
        led.def_at_max_steps += board.cost_def == board.max_cost
        led.atk_at_max_steps += board.cost_atk == board.max_cost
        return reward

    def summon(board, types, road):
        n = len(board.enemies)
        out = summon0(board, types, road)
        led.lv1_summons += sum(e.lv == 1 for e in board.enemies[n:])
        return out

    def lvup(board, loc):
        ok = lvup0(board, loc)
        led.lv0_refused_upgrades += (not ok) and board.fail_code == O.FAIL_LVMAX and board.cfg.max_tower_lv == 0
        return ok

    def destruct(board, loc):
        tw = board._tower_at(loc)
        uncapped = None if tw is None else board.cost_def + tw.cost * board.cfg.tower_destruct_return
        ok = destruct0(board, loc)
        # observed, not re-derived: the board ends at max_cost and the sum it cut was above it
        led.capped_destructs += bool(ok and uncapped > board.max_cost and board.cost_def == board.max_cost)
        return ok

    def env_step(env, def_act=None, atk_act=None):
        out = env_step0(env, def_act, atk_act)
        led.cooldown_over15 += env.attacker_cd > 15 or env.defender_cd > 15
        return out

    O._fire, O.Enemy.hit, O.Board.step, O.Env.step = fire, hit, step, env_step
    O.Board.summon_cluster, O.Board.tower_lvup, O.Board.tower_destruct = summon, lvup, destruct
    try:
        yield led
    finally:
        O._fire, O.Enemy.hit, O.Board.step, O.Env.step = fire0, hit0, step0, env_step0
        O.Board.summon_cluster, O.Board.tower_lvup, O.Board.tower_destruct = summon0, lvup0, destruct0
