"""Crowded and full boards: the scenarios, and an oracle that counts what it did.

Shared by tests/test_crowded_ref.py (CPU: the scenarios still reach what they are meant to
reach), tests/test_gpu_crowded.py (the device against the oracle on them) and
tests/test_gpu_frame_skip_crowded.py (the same at frame skip, SKIP_CASES).  Not a test
module.

The step kernels keep a board's enemies two per lane -- lane l owns list entries l and
l + 64 -- and every phase of the step has a branch of its own for the second entry
(gym-td_amd/csrc td_step_rules.h board_step, td_step_obs.h enemy_stats, td_step_state.h store_enemies).  A scenario is a
game config, a mode and a seeded policy under which the REFERENCE rules put more than 64
enemies (up to exactly 128, the device's capacity) or 32 towers (likewise) on a board;
`Counters` records, from the oracle's own lists, which of those second-half branches a
bit-exact device has to have taken.  All indices are list positions after the step's sort
(what a tower scans, TDBoard.py:305-313), or positions in the list the step leaves behind
(the group heads of the enemy_LP planes, TDBoard.py:355-365).
"""
import contextlib

import numpy as np

from oracle import canon, policies
from oracle import td_oracle as O

ROAD_ATTEMPTS = 1000  # the device's bound of each create_road_v2 loop (td_kernels.h kRoadAttempts)
ENEMY_CAP, TOWER_CAP, HALF = 128, 32, 64  # td_common.h ECAP / TCAP; lanes per wave
FLAG_EN_OVERFLOW, FLAG_TW_OVERFLOW = 1, 2  # include/tdstep.h td_board_flag

_COUNTS = ("hi_steps", "full_steps", "hi_splash", "hi_frozen", "hi_kills", "lo_kill_hi_live", "cross_sort",
           "hi_head", "head_127", "refused_summons", "refused_builds", "full_tower_steps", "full_destructs",
           "full_upgrades", "rebuilds")


class Counters(object):
    """What the oracle did, over the board-steps it was asked to count.

    hi_steps / full_steps  board-steps entered with more than 64 / exactly 128 enemies
    hi_target[t]           shots of tower type t whose target's index is >= 64
    hi_splash              bomb shots that damage an enemy at index >= 64
    hi_frozen              frozen victims at index >= 64
    hi_kills               kills at index >= 64
    lo_kill_hi_live        kills at index < 64 in a step that keeps a survivor at index >= 64
                           (the survivors the compaction moves across the halves)
    cross_sort             enemies whose index before and after the sort lie in different halves
    hi_head / head_127     enemy_LP group heads (first enemy of a (type, cell) in the list the
                           step leaves) at index >= 64 / at index 127
    refused_summons / refused_builds   refusals by a cap
    full_tower_steps       board-steps entered with 32 towers
    full_destructs / full_upgrades     successful destructs / upgrades on a 32-tower list
    rebuilds               successful builds on a board after such a destruct
    max_enemies / max_towers           the longest lists seen (at step entry / after the actions)
    """

    def __init__(self):
        for k in _COUNTS:
            setattr(self, k, 0)
        self.hi_target = [0, 0, 0, 0]
        self.max_enemies = self.max_towers = 0

    def add(self, other):
        for k in _COUNTS:
            setattr(self, k, getattr(self, k) + getattr(other, k))
        self.hi_target = [a + b for a, b in zip(self.hi_target, other.hi_target)]
        self.max_enemies = max(self.max_enemies, other.max_enemies)
        self.max_towers = max(self.max_towers, other.max_towers)
        return self

    def as_dict(self):
        d = {k: getattr(self, k) for k in _COUNTS}
        d.update(hi_target=list(self.hi_target), max_enemies=self.max_enemies, max_towers=self.max_towers)
        return d

    def __repr__(self):
        return "Counters(%s)" % ", ".join("%s=%r" % kv for kv in sorted(self.as_dict().items()))


@contextlib.contextmanager
def counting(cnt):
    """Inside the block the oracle's `_fire`, `Board.step` and the three tower operations
    report to `cnt`.  The wrappers only read; they call the unchanged originals, so a counted
    trajectory is the trajectory."""
    fire0, step0 = O._fire, O.Board.step
    build0, lvup0, destruct0 = O.Board.tower_build, O.Board.tower_lvup, O.Board.tower_destruct

    def fire(tw, enemies, cfg):
        # the target and the victims exactly as _fire picks them (TDElements.py:71-132)
        tgt = next((i for i, e in enumerate(enemies) if O._cheb(e.loc, tw.loc) <= tw.rge), None)
        if tgt is not None:
            if tgt >= HALF:
                cnt.hi_target[tw.type] += 1
            if tw.type >= 2:
                hit = [i for i, e in enumerate(enemies) if O._cheb(enemies[tgt].loc, e.loc) <= tw.dmgrge]
                if tw.type == 2 and hit and hit[-1] >= HALF:
                    cnt.hi_splash += 1
                if tw.type == 3 and hit and hit[0] >= HALF:
                    cnt.hi_frozen += 1
        return fire0(tw, enemies, cfg)

    def step(board):
        before = board.enemies
        n = len(before)
        cnt.max_enemies = max(cnt.max_enemies, n)
        cnt.max_towers = max(cnt.max_towers, len(board.towers))
        cnt.hi_steps += n > HALF
        cnt.full_steps += n == ENEMY_CAP
        cnt.full_tower_steps += len(board.towers) == TOWER_CAP
        # the same stable sort on the same keys as Board.step's (TDBoard.py:305)
        order = sorted(before, key=lambda e: e.dist - e.margin)
        pos = {id(e): i for i, e in enumerate(before)}
        cnt.cross_sort += sum((pos[id(e)] >= HALF) != (i >= HALF) for i, e in enumerate(order))
        reward = step0(board)
        left = set(id(e) for e in board.enemies)
        killed = [i for i, e in enumerate(order) if not e.LP > 0]  # an enemy at LP 0 was hit this step
        cnt.hi_kills += sum(i >= HALF for i in killed)
        if any(id(e) in left for e in order[HALF:]):
            cnt.lo_kill_hi_live += sum(i < HALF for i in killed)
        seen = set()
        for i, e in enumerate(board.enemies):
            g = (e.type, e.loc[0], e.loc[1])
            if g not in seen:
                seen.add(g)
                cnt.hi_head += i >= HALF
                cnt.head_127 += i == ENEMY_CAP - 1
        return reward

    def build(board, t, loc):
        r0 = board.refused[1]
        ok = build0(board, t, loc)
        cnt.refused_builds += board.refused[1] - r0
        if ok and getattr(board, "_full_destructed", False):
            cnt.rebuilds += 1
        return ok

    def lvup(board, loc):
        full = len(board.towers) == TOWER_CAP
        ok = lvup0(board, loc)
        cnt.full_upgrades += bool(ok and full)
        return ok

    def destruct(board, loc):
        full = len(board.towers) == TOWER_CAP
        ok = destruct0(board, loc)
        if ok and full:
            cnt.full_destructs += 1
            board._full_destructed = True
        return ok

    O._fire, O.Board.step = fire, step
    O.Board.tower_build, O.Board.tower_lvup, O.Board.tower_destruct = build, lvup, destruct
    try:
        yield cnt
    finally:
        O._fire, O.Board.step = fire0, step0
        O.Board.tower_build, O.Board.tower_lvup, O.Board.tower_destruct = build0, lvup0, destruct0


# --------------------------------------------------------------------------
# game configs
# --------------------------------------------------------------------------

def _all(v):
    return [[v, v] for _ in range(4)]


# Sustained crowd: a cheap, slow, steady stream of enemies against a defender with an income:
# boards stay between 64 and 128 enemies for hundreds of steps while towers fire into them.
SUSTAINED = dict(attacker_init_cost=20, attacker_cost_init_rate=1.0, attacker_cost_final_rate=1.0,
                 enemy_cost=_all(1), enemy_speed=[[.15, .15], [.15, .15], [.12, .12], [.15, .15]],
                 base_LP=10 ** 6, defender_init_cost=60, defender_cost_rate=2, max_cost=100)
# Exactly full: the attacker can pay for 128 summons in all and earns nothing, so the
# reference's own rules can never hold more than 128 enemies: no cap is needed to compare.
FULL = dict(attacker_init_cost=128, attacker_cost_init_rate=0, attacker_cost_final_rate=0, enemy_cost=_all(1),
            enemy_speed=_all(.03), defender_init_cost=100, defender_cost_rate=3, max_cost=128)
# Overflow: the same with money for 160 summons: the 129th is refused (oracle: enemy_cap).
OVERFLOW = dict(FULL, attacker_init_cost=160, max_cost=160)
# Full tower list: towers block only their 4-neighbourhood and the defender is rich.
TOWERS = dict(tower_distance=1, defender_init_cost=300, max_cost=400, defender_cost_rate=8, base_LP=10 ** 6,
              attacker_init_cost=40, attacker_cost_init_rate=1.5, attacker_cost_final_rate=1.5, enemy_cost=_all(2))


class Scenario(object):
    """One trajectory family: `B` boards of `mode` at side `L` under `cfg` overrides, the
    first seeds from `seed0` whose layout draws, `steps` steps of `policy` on RandomState(rng)."""

    def __init__(self, name, L, mode, cfg, B=8, steps=400, multi=False, difficulty=1, seed0=4000, rng=5,
                 smart=0.8, policy="random", lone_last=False, enemy_cap=None, tower_cap=None, needs=()):
        self.name, self.L, self.mode, self.cfg = name, L, mode, dict(cfg)
        self.B, self.steps, self.multi, self.difficulty = B, steps, multi, difficulty
        self.seed0, self.rng, self.smart, self.policy = seed0, rng, smart, policy
        self.lone_last = lone_last  # the attacker of every fourth board is _lone_last
        self.enemy_cap, self.tower_cap = enemy_cap, tower_cap
        self.needs = tuple(needs)  # counters this scenario must bring above zero by itself

    @property
    def capped(self):
        return self.enemy_cap is not None or self.tower_cap is not None

    def __repr__(self):
        return self.name


# --------------------------------------------------------------------------
# running a scenario on the oracle
# --------------------------------------------------------------------------

def make_envs(scn, enemy_cap="scenario", tower_cap="scenario"):
    """(seeds, envs): the first scn.B seeds from scn.seed0 whose first layout draw succeeds
    (the reference raises on the others), with their oracle envs."""
    ecap = scn.enemy_cap if enemy_cap == "scenario" else enemy_cap
    tcap = scn.tower_cap if tower_cap == "scenario" else tower_cap
    hp = O.Hyper(allow_multiple_actions=scn.multi)
    mode = {"def": O.MODE_DEF, "atk": O.MODE_ATK, "2p": O.MODE_2P}[scn.mode]
    seeds, envs = [], []
    s = scn.seed0
    while len(seeds) < scn.B:
        try:
            envs.append(O.Env(scn.L, mode, scn.difficulty, s, s, O.Config(**scn.cfg), hp,
                              road_attempts=ROAD_ATTEMPTS, enemy_cap=ecap, tower_cap=tcap))
            seeds.append(s)
        except O.RoadGenError:
            pass
        s += 1
    return seeds, envs


def _builder(rng, env):
    """The full-tower-list defender: mostly a build on a free cell (a refused one once the
    list is full), now and then an upgrade or a destruct of a standing tower."""
    L, b = env.L, env._board
    p = rng.random_sample()
    if b.towers and p < 0.25:
        tw = b.towers[rng.randint(len(b.towers))]
        op = 4 if p < 0.15 else 5
        return int(op * L * L + tw.loc[0] * L + tw.loc[1])
    free = np.flatnonzero(b.map[6].reshape(-1) == 0)
    if len(free) == 0:
        return 6 * L * L
    return int(rng.randint(0, 4) * L * L + free[rng.randint(len(free))])


def _multi_builder(rng, env, p=0.02):
    """Multi-action flags: every operation plane sparse (uniform flags would tear down in
    one scan what they build)."""
    L = env.L
    a = (rng.random_sample((6, L, L)) < p).astype(np.int64)
    a[5] &= (rng.random_sample((L, L)) < 0.1).astype(np.int64)
    return a


def _lone_last(rng, env, a, step=None):
    """The attacker that puts a group head at list index 127: sixteen full clusters on road 0
    in the first sixteen steps, types 0-2 only, but for the very last enemy, of type 3.  All
    wait in the start cell at these speeds, the last one last in the sort and alone of its
    type.  Afterwards `a`, the random attacker's action (the draw count stays the same).
    `step`: the number of the step the action is for (default: the board's step counter; at
    frame skip the macro step's, the attacker acting once per macro step)."""
    fill = rng.randint(0, 3, size=8)
    k = env._board.steps if step is None else step
    if k >= ENEMY_CAP // 8:
        return a
    a = np.full((3, 8), 4, dtype=np.int64)
    a[0] = fill
    if k == ENEMY_CAP // 8 - 1:
        a[0, 7] = 3
    return a


def draw_actions(scn, rng, envs, step=None):
    """(def_act, atk_act) of one step for all boards (None where the mode has no such side),
    drawn for every board whether it still runs or not, so that a board's stream does not
    depend on the others' episodes.  `step`: see _lone_last."""
    L = scn.L
    da = aa = None
    if scn.mode != "atk":
        if scn.multi:
            da = np.stack([_multi_builder(rng, o) for o in envs]).astype(np.int64)
        elif scn.policy == "builder":
            da = np.array([_builder(rng, o) for o in envs], dtype=np.int64)
        else:
            da = np.array([policies.discrete_def(rng, L, o._board.map[0], scn.smart) for o in envs], dtype=np.int64)
    if scn.mode != "def":
        aa = np.stack([policies.atk(rng) for _ in envs]).astype(np.int64)
        if scn.lone_last:
            for b in range(3, len(envs), 4):
                aa[b] = _lone_last(rng, envs[b], aa[b], step)
    return da, aa


class Expect(object):
    """What one board must show after one step."""
    __slots__ = ("obs", "reward", "done", "digest", "info", "cds")

    def __init__(self, env, out):
        self.obs, self.reward, self.done, self.info = out
        self.digest = canon.state_digest(canon.oracle_state(env))
        self.cds = (env.attacker_cd, env.defender_cd)


def step_envs(scn, envs, da, aa):
    """One step of every board that still runs: [Expect or None (finished earlier)]."""
    out = []
    for b, o in enumerate(envs):
        if o._board.done():
            out.append(None)
            continue
        d_b = None if da is None else (da[b] if scn.multi else int(da[b]))
        out.append(Expect(o, o.step(d_b, None if aa is None else aa[b])))
    return out


def macro_step_envs(scn, envs, da, aa, k):
    """One macro step at frame skip k of every board that still runs: the actions at sub-step
    0, then the empty ones, stopped after the sub-step that ends the episode.  The Expect is
    taken after the last sub-step run, with the rewards summed left to right; RealAction and
    FailCode are sub-step 0's."""
    assert not scn.multi  # (multi-action handles refuse k > 1)
    out = []
    for b, o in enumerate(envs):
        if o._board.done():
            out.append(None)
            continue
        total = first = res = None
        for j in range(k):
            d = None if da is None else (int(da[b]) if j == 0 else o.empty_def())
            a = None if aa is None else (aa[b] if j == 0 else o.empty_atk())
            res = o.step(d, a)
            total = res[1] if j == 0 else total + res[1]
            first = res[3] if j == 0 else first
            if res[2]:
                break
        info = dict(res[3], RealAction=first["RealAction"], FailCode=first["FailCode"])
        out.append(Expect(o, (res[0], total, res[2], info)))
    return out


class Reference(object):
    """A scenario run once on the oracle: seeds, per-step actions and expectations, the
    counters, and per board the refusals ([summons, builds]) and the longest lists.

    At frame skip k > 1 the scenario's board steps are run as ``steps // k`` macro steps: the
    policy's actions are drawn once per macro step, ``steps`` holds one entry per macro step
    and the counters count every sub-step."""

    def __init__(self, scn, k=1):
        self.scn, self.k = scn, k
        self.seeds, envs = make_envs(scn)
        self.counters = Counters()
        self.steps = []
        self.n_enemies = []  # per step, per board: enemies left after the step (-1: not running)
        rng = np.random.RandomState(scn.rng)
        with counting(self.counters):
            for i in range(scn.steps // k):
                da, aa = draw_actions(scn, rng, envs, None if k == 1 else i)
                want = step_envs(scn, envs, da, aa) if k == 1 else macro_step_envs(scn, envs, da, aa, k)
                self.steps.append((da, aa, want))
                self.n_enemies.append([len(o._board.enemies) if w is not None else -1 for o, w in zip(envs, want)])
        self.refused = [list(o.refused) for o in envs]
        self.counters.refused_summons = sum(r[0] for r in self.refused)
        self.running = sum(not o._board.done() for o in envs)

    def flags(self):
        """The device's flag word of each board: a cap refusal, nothing else."""
        return [FLAG_EN_OVERFLOW * (r[0] > 0) | FLAG_TW_OVERFLOW * (r[1] > 0) for r in self.refused]


_cache = {}


def reference(scn, k=1):
    """The scenario's Reference, computed once and shared (the last one is kept: the tests
    of one scenario on the three step kernels run back to back)."""
    if (scn.name, k) not in _cache:
        _cache.clear()
        _cache[(scn.name, k)] = Reference(scn, k)
    return _cache[(scn.name, k)]


# --------------------------------------------------------------------------
# the scenarios, and what each has to reach by itself
# --------------------------------------------------------------------------
# `needs` are floors on the oracle's own counters, well below what the CPU runs that chose
# the seeds gave (listed in tests/test_crowded_ref.py): they keep a comparison on the
# scenario from passing after the scenario has drifted away from the branch it is there for.
_CROWD = ("cross_sort", "lo_kill_hi_live", "hi_head", "hi_frozen", "hi_target[3]")
_FULL = _CROWD + ("hi_kills", "hi_splash", "hi_target[1]")

SCENARIOS = [
    Scenario("sustained-2p", 10, "2p", SUSTAINED, steps=300, seed0=4000,
             needs=_CROWD + ("hi_target[0]", "hi_target[1]", ("hi_steps", 800))),
    Scenario("sustained-atk", 10, "atk", SUSTAINED, steps=300, seed0=4100,
             needs=_CROWD + ("hi_kills", "hi_splash", "hi_target[2]", ("hi_steps", 800))),
    Scenario("full-atk", 10, "atk", FULL, steps=200, seed0=4200, lone_last=True,
             needs=_FULL + ("head_127", ("full_steps", 20), ("hi_steps", 500))),
    Scenario("full-def", 10, "def", FULL, steps=200, seed0=4300,
             needs=_FULL + ("hi_target[2]", ("full_steps", 20), ("hi_steps", 500))),
    Scenario("full-2p-20", 20, "2p", FULL, steps=200, multi=True, seed0=4400, rng=7, lone_last=True,
             tower_cap=TOWER_CAP,
             needs=_FULL + ("hi_target[0]", "hi_target[2]", "head_127", ("full_steps", 20), ("hi_steps", 500),
                            ("full_tower_steps", 100), "refused_builds", "full_destructs", "full_upgrades", "rebuilds")),
    Scenario("full-atk-12", 12, "atk", FULL, steps=200, seed0=4500, lone_last=True,
             needs=_FULL + ("hi_target[0]", "hi_target[2]", "head_127", ("full_steps", 20), ("hi_steps", 500))),
    Scenario("overflow-atk", 10, "atk", OVERFLOW, steps=200, seed0=4600, enemy_cap=ENEMY_CAP,
             needs=_FULL + ("hi_target[0]", "hi_target[2]", "head_127", ("full_steps", 100), "refused_summons")),
    Scenario("overflow-2p", 10, "2p", OVERFLOW, steps=200, seed0=4700, enemy_cap=ENEMY_CAP,
             needs=_FULL + ("hi_target[0]", "head_127", ("full_steps", 100), "refused_summons")),
    Scenario("towers-def", 10, "def", TOWERS, steps=200, seed0=4800, policy="builder", tower_cap=TOWER_CAP,
             needs=(("full_tower_steps", 200), "refused_builds", "full_destructs", "full_upgrades", "rebuilds")),
]
BY_NAME = {s.name: s for s in SCENARIOS}

# Frame skip on the same boards: (scenario, k) at which the Python oracle, with the scenario's
# own seeds and the actions once per macro step, still holds every floor of the scenario's
# `needs` unchanged.  overflow-2p at k = 2 reaches neither a frozen victim nor a freezer's target
# in the upper half (0 for both; the other rows cover them): its floors less those two.
# full-2p-20 is multi-action, which refuses k > 1.
SKIP_CASES = [("sustained-2p", 2), ("sustained-atk", 2), ("sustained-atk", 4), ("full-atk", 2), ("full-def", 2),
              ("full-def", 4), ("full-atk-12", 2), ("overflow-atk", 2), ("overflow-atk", 4), ("towers-def", 2),
              ("overflow-2p", 2)]
SKIP_DROPPED = {("overflow-2p", 2): ("hi_frozen", "hi_target[3]")}


def counter(cnt, key):
    if key.startswith("hi_target["):
        return cnt.hi_target[int(key[10])]
    return getattr(cnt, key)


def check_scenario(ref):
    """The scenario's own conditions on the oracle's counters (raises AssertionError)."""
    scn, cnt = ref.scn, ref.counters
    dropped = SKIP_DROPPED.get((scn.name, ref.k), ())
    for need in scn.needs:
        key, floor = need if isinstance(need, tuple) else (need, 1)
        if key in dropped:
            continue
        assert counter(cnt, key) >= floor, (scn.name, key, counter(cnt, key), floor)
    # what no cap stands behind, the reference's own rules have to keep within the device's lists
    if scn.enemy_cap is None:
        assert cnt.max_enemies <= ENEMY_CAP and cnt.refused_summons == 0, (scn.name, cnt.max_enemies)
    if scn.tower_cap is None:
        assert cnt.max_towers <= TOWER_CAP and cnt.refused_builds == 0, (scn.name, cnt.max_towers)
    else:
        assert cnt.max_towers == TOWER_CAP, (scn.name, cnt.max_towers)
    if scn.enemy_cap is not None:  # the overflow is met on at least half of the boards
        assert 2 * sum(r[0] > 0 for r in ref.refused) >= scn.B, (scn.name, ref.refused)
