"""Hand-made maps: the catalogue, its oracle and the run both test files drive
(tests/test_hand_layout_ref.py on the CPU oracle alone, tests/test_gpu_hand_layouts.py on the
device).  Not a test module.

Every other board the suite steps runs on roads create_road_v2 drew.  These come through the
caller's path instead -- td_layout_from_roads + td_reset_layouts -- and are drawn to reach what
generated roads never do: a road of exactly 64 cells (the last entry of the step kernels'
distance table), roads along the board's edges, a road that overwrites another road's
distances and directions, roads of 2 and 3 cells, and boards of 4, 5 and 6 cells a side.

The layout rule (include/tdstep.h): each road is a simple 4-connected path of 2..64 cells,
and every road leads into road 0's last cell."""
import numpy as np

from oracle import policies
from oracle import td_oracle as O

MODES = {"def": O.MODE_DEF, "atk": O.MODE_ATK, "2p": O.MODE_2P}
STEP = {"R": (0, 1), "L": (0, -1), "D": (1, 0), "U": (-1, 0)}


def path(start, moves):
    """The cells of a walk: ``start`` (row, col), then e.g. "U9 R1 D9": 9 up, 1 right, 9 down."""
    r, c = start
    cells = [(r, c)]
    for m in moves.split():
        dr, dc = STEP[m[0]]
        for _ in range(int(m[1:])):
            r, c = r + dr, c + dc
            cells.append((r, c))
    return cells


def check_roads(roads, L):
    """The layout rule, asserted on a map of the catalogue."""
    for road in roads:
        assert 2 <= len(road) <= 64 and len(set(road)) == len(road), road
        assert all(0 <= r < L and 0 <= c < L for r, c in road), road
        assert all(abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 for a, b in zip(road, road[1:])), road
        assert road[-1] == roads[0][-1], road


def try_record(roads, L, rec=None):
    """td_layout_from_roads, into ``rec`` if given: (return code, record)."""
    from gym_TD import _lib
    cells = np.asarray([p[0] * L + p[1] for r in roads for p in r] + [0], dtype=np.int32)  # (never empty)
    off = np.cumsum([0] + [len(r) for r in roads]).astype(np.int32)
    rec = np.zeros(8 + L * L, np.uint32) if rec is None else rec
    rc = _lib.lib.td_layout_from_roads(L, len(roads), _lib.ptr(cells, _lib.ctypes.c_int32),
                                       _lib.ptr(off, _lib.ctypes.c_int32), _lib.ptr(rec, _lib.ctypes.c_uint32))
    return rc, rec


def record(roads, L):
    """The layout record of ``roads`` (lists of (row, col))."""
    rc, rec = try_record(roads, L)
    assert rc == 0, (rc, roads)
    return rec


# --------------------------------------------------------------------------
# the oracle
# --------------------------------------------------------------------------

class TracedBoard(O.Board):
    """O.Board that also counts, into ``trace`` (shared with the env, so it outlives a reset),
    what the catalogue's maps are there to reach.  It changes no rule."""

    def __init__(self, *a, **kw):
        self.trace = kw.pop("trace")
        O.Board.__init__(self, *a, **kw)
        self._road_of = {}  # id(enemy) -> (road, enemy): the reference keeps the enemy's id alive

    def summon_cluster(self, types, road):
        n = len(self.enemies)
        out = O.Board.summon_cluster(self, types, road)
        for e in self.enemies[n:]:
            self._road_of[id(e)] = (road, e)
        return out

    def tower_build(self, t, loc):
        ok = O.Board.tower_build(self, t, loc)
        k = self.cfg.tower_distance
        if ok and (min(loc) < k or max(loc) > self.L - 1 - k):
            self.trace["clipped_towers"] += 1
        if not ok and self.fail_code == O.FAIL_POS:
            self.trace["fail_pos"] += 1
        return ok

    def step(self):
        tr, m = self.trace, self.map
        before = [(e, list(e.loc)) for e in self.enemies]
        lp = self.base_LP
        reward = O.Board.step(self)
        tr["leaks"] += lp - self.base_LP
        move = ((0, 1), (0, -1), (1, 0), (-1, 0))
        for e, p in before:
            dirs = []
            while p != list(e.loc) and len(dirs) < 8:  # (an enemy moves at most 3 cells: follow map[5])
                d = int(m[5, p[0], p[1]])
                dirs.append(d)
                p = [p[0] + move[d][0], p[1] + move[d][1]]
            tr["dirs"].update(dirs)
            if len(dirs) >= 2 and len(set(dirs)) >= 2:
                tr["turn_steps"] += 1
        far = int(m[4].max())
        for e in self.enemies:
            r, c = e.loc
            if m[4, r, c] == far:
                tr["on_maxdist"] += 1
            if self._road_of[id(e)][0] == 0 and m[1, r, c] == 0 and m[2, r, c] == 1:
                tr["road0_on_road1_only"] += 1
        return reward


def new_trace():
    return dict(leaks=0, dirs=set(), turn_steps=0, on_maxdist=0, road0_on_road1_only=0, clipped_towers=0,
                fail_pos=0, episodes=0, ends_by_leak=0, ends_by_limit=0)


class HandEnv(O.Env):
    """O.Env on caller-made roads, as td_reset_layouts restarts a board: the layout is given,
    so reset() draws nothing from ``np_random``, and the opponent's stream runs on across
    resets.  The list capacities are the device's (128 enemies, 32 towers)."""

    def __init__(self, roads, L, mode, difficulty, opp_seed, cfg, hp, stay_on_bad_move=False):
        self.roads = [[list(p) for p in r] for r in roads]  # (before O.Env.__init__ calls reset())
        self.stay_on_bad_move = stay_on_bad_move
        self.trace = new_trace()
        O.Env.__init__(self, L, mode, difficulty, 0, opp_seed, cfg, hp, enemy_cap=128, tower_cap=32)

    def reset(self):
        self.num_roads = len(self.roads)
        self._board = TracedBoard(self.L, self.num_roads, None, self.cfg, self.hp, roads=self.roads, enemy_cap=128,
                                  tower_cap=32, refused=self.refused, stay_on_bad_move=self.stay_on_bad_move,
                                  trace=self.trace)
        self.attacker_cd = 0
        self.defender_cd = 0
        return self._board.get_states()


# --------------------------------------------------------------------------
# the maps
# --------------------------------------------------------------------------

_MERGE3_ROAD0 = path((1, 1), "R12 D12 L4 D3")  # ends in (16, 9)

MAPS = {
    # one serpentine of exactly 64 cells: max dist 63, every direction code
    "snake64": (10, [path((9, 0), "U9 R1 D9 R1 U9 R1 D9 R6 U1 L5 U1 R5 U1 L5")]),
    # three edges through two corners, and the fourth edge
    "border": (10, [path((0, 0), "R9 D9 L9"), path((1, 0), "D8")]),
    # road 0 a detour; road 1 through road 0's start, then straight: it overwrites the distance
    # (17 -> 9) and the direction of that cell, so road-0 enemies walk road 1
    "cross": (12, [path((6, 1), "U4 R8 D4 R1"), path((11, 1), "L1 U5 R10")]),
    # three roads joining at different cells, all four direction codes between them
    "merge3": (20, [_MERGE3_ROAD0, path((18, 2), "U5 R7 D3"), path((8, 19), "L6 D5 L4 D3")]),
    # a 2-cell road (the first move leaks) and a 3-cell one round a corner
    "two": (10, [[(4, 4), (4, 5)], path((5, 6), "L1 U1")]),
    "tiny4": (4, [path((0, 0), "D3 R3")]),
    "tiny5": (5, [path((0, 4), "L4 D4")]),
    "tiny6": (6, [path((0, 0), "R5 D5"), path((3, 0), "R5 D2")]),
    # road 1 dead-ends on the right edge: its last cell's default direction (+c) points off the
    # board.  Against the layout rule on purpose (TD_FLAG_BAD_MOVE); not part of CASES.
    "deadend": (10, [path((1, 1), "D7 R5"), [(5, 8), (5, 9)]]),
}

SPEED = [[2.5, 2.5], [1.0, 1.0], [0.5, 0.5], [0.25, 0.25]]  # cells per step: 2.5 rounds corners, 1.0 is the margin >= 1 edge
EPISODE_STEPS = 40


def config(**over):
    """Fast enemies, incomes on both sides and a 3-point base: episodes end by leaks and by the
    40-step limit (hyper()) inside a run of 60-150 steps."""
    d = dict(enemy_speed=[list(x) for x in SPEED], enemy_cost=[[4, 4], [6, 6], [10, 10], [8, 8]], base_LP=6,
             attacker_init_cost=40, attacker_cost_init_rate=6, attacker_cost_final_rate=8, defender_init_cost=20,
             defender_cost_rate=1.0, tower_distance=2)
    d.update(over)
    return O.Config(**d)


def hyper():
    hp = O.Hyper()
    hp.max_episode_steps = EPISODE_STEPS
    return hp


# (name of the case, map, mode, difficulty of the built-in opponent, config overrides, boards, steps)
CASES = [
    ("snake64", "snake64", "atk", 1, {}, 12, 120),
    ("border", "border", "def", 1, {}, 12, 100),
    ("cross", "cross", "atk", 2, {}, 12, 100),
    ("merge3", "merge3", "2p", 1, {}, 8, 100),
    ("two", "two", "atk", 1, {}, 8, 80),
    ("tiny4", "tiny4", "atk", 0, {}, 8, 80),
    ("tiny4-d1", "tiny4", "atk", 0, dict(tower_distance=1), 8, 80),
    ("tiny5", "tiny5", "atk", 0, {}, 8, 80),
    ("tiny6", "tiny6", "atk", 0, {}, 8, 80),
]
CASE = {c[0]: c for c in CASES}
OPP_SEED0 = 100  # board b's opponent stream: random.Random(OPP_SEED0 + b)


def make_envs(case, n=None, stay_on_bad_move=False):
    """(L, roads, the case's HandEnvs) -- board b's opponent seeded OPP_SEED0 + b."""
    _, name, mode, difficulty, over, boards, _ = CASE[case]
    L, roads = MAPS[name]
    n = boards if n is None else n
    return L, roads, [HandEnv(roads, L, MODES[mode], difficulty, OPP_SEED0 + b, config(**over), hyper(),
                              stay_on_bad_move=stay_on_bad_move) for b in range(n)]


def draw_actions(rng, mode, envs, L):
    """One step's caller actions (def [B] or None, atk [B, 3, 8] or None): the defender builds
    near the road half of the time, the attacker places enemies on every road."""
    da = aa = None
    if mode != "atk":
        da = np.array([policies.discrete_def(rng, L, o._board.map[0], 0.5) for o in envs], dtype=np.int64)
    if mode != "def":
        aa = np.stack([policies.atk(rng) for _ in envs]).astype(np.int64)
    return da, aa


def note_end(env):
    """Count a finished episode into the env's trace (before it is reset)."""
    b, tr = env._board, env.trace
    tr["episodes"] += 1
    if b.base_LP <= 0:
        tr["ends_by_leak"] += 1
    else:
        tr["ends_by_limit"] += 1


def merged_trace(envs):
    out = new_trace()
    for o in envs:
        for k, v in o.trace.items():
            if isinstance(v, set):
                out[k] |= v
            else:
                out[k] += v
    out["refused"] = [sum(o.refused[i] for o in envs) for i in (0, 1)]
    return out


def run_envs(envs, mode, L, steps):
    """``steps`` steps of draw_actions on oracle envs alone, finished boards restarted as the
    GPU tests restart them: the merged trace."""
    rng = np.random.RandomState(L)
    for _ in range(steps):
        da, aa = draw_actions(rng, mode, envs, L)
        for b, o in enumerate(envs):
            _, _, done, _ = o.step(None if da is None else int(da[b]), None if aa is None else aa[b])
            if done:
                note_end(o)
                o.reset()
    return merged_trace(envs)


def run_oracle(case):
    """The case's run on the oracle alone."""
    L, _, envs = make_envs(case)
    return run_envs(envs, CASE[case][2], L, CASE[case][6])


# TD_FLAG_BAD_MOVE: TD-atk, 10x10, 8 boards, even boards on `border`, odd boards on `deadend`
BAD_MOVE_BOARDS, BAD_MOVE_STEPS = 8, 100


def bad_move_envs():
    """(L, [the roads of board b], envs with the device's rule for a move off the board)."""
    L = 10
    roads = [MAPS["deadend" if b % 2 else "border"][1] for b in range(BAD_MOVE_BOARDS)]
    return L, roads, [HandEnv(r, L, O.MODE_ATK, 1, OPP_SEED0 + b, config(), hyper(), stay_on_bad_move=True)
                      for b, r in enumerate(roads)]
