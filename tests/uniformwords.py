"""The cases of tests/test_gpu_uniform_words.py and tests/test_uniform_words_ref.py, and an oracle
ledger of what they reach.  Not a test module.

The step kernels take three short cuts through a board's common path (gym-td_amd/csrc
td_step_rules.h): a summon's enemy level is an integer test on the step count (td_upgrade_step.h),
a cluster of eight equal types is summoned by one loop that stops at the first slot that fails,
and a board without an enemy skips kills, march, leaks and compaction (the two-wave kernels
take the first only and keep the unrolled cluster and the whole board step).  A case is a game config, a
mode and a seeded policy under which the REFERENCE rules walk those branches; `Ledger` counts,
from the oracle's own calls, which of them a bit-exact device has to have taken, and a case names
the events it must reach by itself (`needs`): a run that did not is refused.
"""
import contextlib
import copy

import numpy as np

from oracle import policies
from oracle import td_oracle as O

ROAD_ATTEMPTS = 1000  # the device's bound of each create_road_v2 loop (td_kernels.h kRoadAttempts)
ENEMY_CAP = 128       # td_common.h ECAP
B = 37                # xcd_board's remainder branch (37 = 8 * 4 + 5)
MODES = {"def": O.MODE_DEF, "atk": O.MODE_ATK, "2p": O.MODE_2P}

_EVENTS = ("all4", "mixed", "cost_mid", "cap_mid", "cap_first", "lv0_summons", "lv1_summons", "first_enemy",
           "last_enemy", "empty_steps", "past_limit_steps", "past_limit_summons")


class Ledger(object):
    """What the oracle did:

    same[m]            clusters of eight equal types (not all 4) of which m slots were summoned, m = 0..8
    all4 / mixed       clusters of eight 4s / of unequal types
    cost_mid           equal-type clusters stopped by the cost after at least one summon
    cap_mid / cap_first   equal-type clusters stopped by the full list after at least one summon / at slot 0
    lv0 / lv1_summons  enemies summoned at level 0 / 1
    first_enemy        clusters that put the first enemy on an empty board
    last_enemy         board steps that began with enemies and left none
    empty_steps        board steps without an enemy
    past_limit_steps / past_limit_summons   board steps / summons at steps >= max_episode_steps"""

    def __init__(self):
        self.same = [0] * 9
        for k in _EVENTS:
            setattr(self, k, 0)

    def get(self, key):
        return self.same[int(key[5])] if key.startswith("same[") else getattr(self, key)

    def __repr__(self):
        return "Ledger(same=%r, %s)" % (self.same, ", ".join("%s=%d" % (k, getattr(self, k)) for k in _EVENTS))


@contextlib.contextmanager
def counting(led):
    """Inside the block Board.summon_cluster and Board.step report to `led`.  The wrappers only
    read; they call the unchanged originals."""
    summon0, step0 = O.Board.summon_cluster, O.Board.step

    def summon(board, types, road):
        types = [int(t) for t in types]
        n0, refused0 = len(board.enemies), board.refused[0]
        res = summon0(board, types, road)
        m = len(board.enemies) - n0
        if all(t == 4 for t in types):
            led.all4 += 1
        elif len(set(types)) == 1:
            led.same[m] += 1
            capped = board.refused[0] > refused0
            led.cap_mid += capped and m > 0
            led.cap_first += capped and m == 0
            led.cost_mid += (not capped) and 0 < m < 8
        else:
            led.mixed += 1
        if m:
            lv1 = sum(e.lv for e in board.enemies[n0:])
            led.lv1_summons += lv1
            led.lv0_summons += m - lv1
            led.first_enemy += n0 == 0
            led.past_limit_summons += m * (board.steps >= board.hp.max_episode_steps)
        return res

    def step(board):
        n0 = len(board.enemies)
        led.empty_steps += n0 == 0
        led.past_limit_steps += board.steps >= board.hp.max_episode_steps
        res = step0(board)
        led.last_enemy += n0 > 0 and not board.enemies
        return res

    O.Board.summon_cluster, O.Board.step = summon, step
    try:
        yield led
    finally:
        O.Board.summon_cluster, O.Board.step = summon0, step0


def _pairs(lv0, lv1):
    return [[a, b] for a, b in zip(lv0, lv1)]


# Enemies that a few towers kill and that cross a 10x10 map in a dozen steps: boards empty out.
_WEAK = dict(enemy_LP=_pairs([200, 400, 900, 700], [300, 600, 1200, 1000]),
             enemy_speed=_pairs([.75, .5, .375, .5], [.75, .5, .375, .5]))
# Built-in lv1 attacker, paid every third step: between its clusters cost_atk grows past the
# price of 0 .. 8 enemies of the type drawn.  Prices with fractions, dearer at level 1; the level
# changes at progress 0.5 of a 60-step episode, and the base outlives the episode limit.
CLUSTERS = dict(enemy_cost=_pairs([2.5, 4.25, 13.75, 9.125], [3.5, 6.5, 20.25, 12.0625]), attacker_init_cost=7.5,
                attacker_cost_init_rate=2.25, attacker_cost_final_rate=3.125, attacker_action_interval=3,
                enemy_upgrade_at=0.5, base_LP=10 ** 6, defender_init_cost=60, defender_cost_rate=2, **_WEAK)
# A list that fills up in the middle of a cluster: 150 to spend on enemies at 0.5 .. 1.5 that hardly move.
FILL = dict(enemy_cost=_pairs([.5, .75, 1.25, 1.5], [.5, .75, 1.25, 1.5]), attacker_init_cost=150, max_cost=150,
            attacker_cost_init_rate=0.5, attacker_cost_final_rate=0.5, enemy_speed=_pairs([.03] * 4, [.03] * 4),
            base_LP=10 ** 6, defender_init_cost=100, defender_cost_rate=3)
# A caller's attacker: an income that pays for some slots of most clusters.
CALLER = dict(enemy_cost=_pairs([3, 5.5, 9, 7.25], [4, 7.5, 12, 9.25]), attacker_init_cost=12, attacker_cost_init_rate=1.5,
              attacker_cost_final_rate=2.75, attacker_action_interval=3, enemy_upgrade_at=0.4, base_LP=10 ** 6,
              defender_init_cost=60, defender_cost_rate=2, **_WEAK)


class Case(object):
    """`steps` steps of B boards of `mode` at 10x10 under `cfg` overrides and an episode limit
    `limit`, auto-reset off.  `kernels`: the step kernels the device runs it on; `variants`:
    further device runs on the last of them ("f16", "skip3", "twin": against a retain_obs=False
    engine).  `switch`: {step: (cfg overrides, limit)} -- td_set_config before that step.
    `past`: boards keep being stepped past the episode limit (never past a fallen base)."""

    def __init__(self, name, mode, cfg, limit, steps, kernels=("small",), variants=(), needs=(), multi=False,
                 difficulty=1, switch=None, past=False, enemy_cap=None, seed0=8100, rng=3):
        self.name, self.mode, self.cfg_ov, self.limit, self.steps = name, mode, dict(cfg), limit, steps
        self.kernels, self.variants, self.needs = tuple(kernels), tuple(variants), tuple(needs)
        self.multi, self.difficulty, self.switch, self.past = multi, difficulty, dict(switch or {}), past
        self.enemy_cap, self.seed0, self.rng = enemy_cap, seed0, rng

    def __repr__(self):
        return self.name


_ALL_COUNTS = tuple("same[%d]" % m for m in range(9))
_EMPTY = ("first_enemy", "last_enemy", ("empty_steps", 100))
_EMPTY_FEW = (("first_enemy", 50), ("last_enemy", 10), ("empty_steps", 20))

CASES = [
    # 0, 1 .. 7 and 8 slots succeed; the cost stops a cluster in the middle; fractions in enemy_cost;
    # episodes cross enemy_upgrade_at with level-1 prices that differ; stepped past the limit
    Case("def-clusters", "def", CLUSTERS, 60, 80, kernels=("small", "small2", "large"), variants=("f16", "skip3", "twin"),
         past=True, needs=_ALL_COUNTS + _EMPTY + ("cost_mid", ("lv0_summons", 100), ("lv1_summons", 100),
                                                  ("past_limit_steps", 500), ("past_limit_summons", 50))),
    # the full list stops a cluster in the middle (and, later, at its first slot)
    Case("def-fill", "def", FILL, 1200, 45, kernels=("small", "large"), enemy_cap=ENEMY_CAP, seed0=8200,
         needs=("cap_mid", "cap_first", "cost_mid", "same[8]")),
    # thresholds 0, 1.0 (the episode's last step count only) and 2.0 (never inside the episode)
    Case("def-up0", "def", dict(CLUSTERS, enemy_upgrade_at=0.0), 30, 40, past=True, seed0=8300,
         needs=(("lv1_summons", 100), "past_limit_summons")),
    Case("def-up1", "def", dict(CLUSTERS, enemy_upgrade_at=1.0), 30, 40, past=True, seed0=8300,
         needs=(("lv0_summons", 100), ("lv1_summons", 20), "past_limit_summons")),
    Case("def-up2", "def", dict(CLUSTERS, enemy_upgrade_at=2.0), 30, 70, past=True, seed0=8300,
         needs=(("lv0_summons", 100), ("lv1_summons", 20), "past_limit_summons")),
    # the caller's clusters: equal types, all 4 and mixed ones, one cluster per road
    Case("atk-caller", "atk", CALLER, 60, 50, kernels=("small", "large"), seed0=8400,
         needs=_ALL_COUNTS[:5] + _EMPTY_FEW + (("mixed", 100), "cost_mid", ("lv0_summons", 50),
                                          ("lv1_summons", 50))),
    Case("2p-caller", "2p", CALLER, 60, 50, kernels=("small2", "large"), seed0=8500,
         needs=_ALL_COUNTS[:5] + _EMPTY_FEW + (("mixed", 100), "cost_mid", ("lv0_summons", 50),
                                          ("lv1_summons", 50))),
    Case("2p-multi", "2p", CALLER, 50, 30, multi=True, seed0=8600, needs=(("all4", 50), ("mixed", 50), "same[0]", "same[1]")),
    # td_set_config in the middle of the episodes: the threshold moves below, then above the
    # boards' progress; then the episode limit shrinks (progress jumps, level 1 again) and grows
    # (`past`: the boards are stepped through the stretch in which the shrunken limit calls them done)
    Case("def-switch", "def", CLUSTERS, 60, 60, kernels=("small", "large"), seed0=8700, past=True,
         switch={20: (dict(enemy_upgrade_at=0.25), 60), 30: (dict(enemy_upgrade_at=0.875), 60),
                 40: (dict(), 45), 50: (dict(), 200)},
         needs=(("lv0_summons", 100), ("lv1_summons", 100))),
]
CASE = {c.name: c for c in CASES}


def hyper(case, limit=None):
    hp = O.Hyper(allow_multiple_actions=case.multi)
    hp.max_episode_steps = case.limit if limit is None else limit
    return hp


def make_envs(case):
    """(seeds, envs, cfg, hp): the first B seeds from case.seed0 whose layout draws; the envs
    share `cfg` and `hp`, so a switch changes them in place (live enemies keep what they captured)."""
    cfg, hp = O.Config(**copy.deepcopy(case.cfg_ov)), hyper(case)
    seeds, envs, s = [], [], case.seed0
    while len(seeds) < B:
        try:
            envs.append(O.Env(10, MODES[case.mode], case.difficulty, s, s, cfg, hp, road_attempts=ROAD_ATTEMPTS,
                              enemy_cap=case.enemy_cap))
            seeds.append(s)
        except O.RoadGenError:
            pass
        s += 1
    return seeds, envs, cfg, hp


def apply_switch(case, k, cfg, hp):
    """The switch before step k, if any, applied to the envs' shared records: True if there is one."""
    if k not in case.switch:
        return False
    ov, limit = case.switch[k]
    for key, v in ov.items():
        setattr(cfg, key, copy.deepcopy(v))
    hp.max_episode_steps = limit
    return True


def _clusters(rng):
    """A caller's attacker action: per road all 4s, eight equal types, or a random cluster."""
    a = policies.atk(rng)
    for road in range(3):
        p = rng.random_sample()
        if p < 0.3:
            a[road] = 4
        elif p < 0.7:
            a[road] = rng.randint(0, 4)
    return a


def draw_actions(case, rng, envs):
    """One step's caller actions for all boards, drawn for every board whether it still runs."""
    da = aa = None
    if case.mode != "atk":
        if case.multi:
            da = np.stack([(rng.random_sample((6, 10, 10)) < 0.02).astype(np.int64) for _ in envs])
        else:
            da = np.array([policies.discrete_def(rng, 10, o._board.map[0], 0.8) for o in envs], dtype=np.int64)
    if case.mode != "def":
        aa = np.stack([_clusters(rng) for _ in envs]).astype(np.int64)
    return da, aa


def act_of(case, da, aa, b):
    d = None if da is None else (da[b] if case.multi else int(da[b]))
    return d, (None if aa is None else aa[b])


def live(case, envs):
    """The boards the next step is compared on: not finished -- or, with `past`, finished by
    the step count alone."""
    if case.past:
        return [b for b, o in enumerate(envs) if o._board.base_LP > 0]
    return [b for b, o in enumerate(envs) if not o._board.done()]


def macro(o, k, d, a):
    """k board steps of oracle env `o` as one macro step: the action, then empty actions, stopped
    at done; the rewards summed left to right; RealAction / FailCode of the first board step."""
    total, first = 0.0, None
    for j in range(k):
        ob, r, done, info = o.step(d if j == 0 else (o.empty_def() if d is not None else None),
                                   a if j == 0 else (o.empty_atk() if a is not None else None))
        total = r if j == 0 else total + r
        first = first or info
        if done:
            break
    return ob, total, done, dict(first, Win=info["Win"], AllowNextMove=info["AllowNextMove"])


def check_needs(case, led):
    for need in case.needs:
        key, floor = need if isinstance(need, tuple) else (need, 1)
        assert led.get(key) >= floor, (case.name, key, led.get(key), floor, led)
