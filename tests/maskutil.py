"""Shared pieces of the action-mask tests (tests/test_action_mask_ref.py on the CPU oracle,
tests/test_gpu_action_mask.py on the device): the game configs, the mask-driven policies
and the oracle-side state record.  Not a test module."""
import numpy as np

from oracle import canon
from oracle import td_oracle as O

ROAD_ATTEMPTS = 1000  # the device's bound of each create_road_v2 loop (td_kernels.h kRoadAttempts)

# "rich": money and a cool-down, so that all six operation classes, every fail code 0-4 and
# cool-down-blocked steps occur within a few hundred steps of the policy below
RICH = dict(defender_init_cost=60, defender_cost_rate=2.0, defender_action_interval=3, tower_distance=1)
# "cap": towers cost 1 and block only their own cell, so the device reaches its 32-tower capacity
CAP = dict(defender_init_cost=1000, max_cost=1000, tower_cost=[[1, 1]] * 4, tower_distance=0)
# attacker: a cool-down, money from the start, and a level-1 price that differs from level 0
ATK = dict(attacker_init_cost=20, attacker_action_interval=3,
           enemy_cost=[[8, 15], [15, 22], [40, 47], [30, 37]])
# 128 live enemies within ~20 steps: everything costs 1 and nobody reaches the base
CROWD = dict(enemy_cost=[[1, 1]] * 4, attacker_init_cost=1000, max_cost=1000, enemy_speed=[[.01, .01]] * 4)


def config(*parts, **kw):
    d = {}
    for p in parts:
        d.update(p)
    d.update(kw)
    return O.Config(**d)


def hyper(multi=False, max_episode_steps=None):
    hp = O.Hyper(allow_multiple_actions=multi)
    if max_episode_steps is not None:
        hp.max_episode_steps = max_episode_steps
    return hp


def ok_seeds(L, n, start, mode, multi=False, difficulty=1, cfg=None, hp=None):
    """The first n seeds from `start` whose first layout draw succeeds (the reference raises
    on the others), with their oracle envs."""
    seeds, envs = [], []
    s = start
    while len(seeds) < n:
        try:
            envs.append(O.Env(L, mode, difficulty, s, s, cfg or O.Config(), hp or hyper(multi),
                              road_attempts=ROAD_ATTEMPTS))
            seeds.append(s)
        except O.RoadGenError:
            pass
        s += 1
    return seeds, envs


def hand_layouts_7():
    """Two 7x7 layout records (td_layout_from_roads): create_road_v2 cannot draw a 7x7 map
    (its randint ranges are empty below L = 8), so boards of that size start from caller
    layouts -- one straight road, and two roads that merge."""
    from gym_TD import _lib
    L = 7
    straight = [[(3, c) for c in range(7)]]
    top = [(1, c) for c in range(7)]
    merge = [top, [(5, 0), (5, 1), (5, 2), (5, 3), (4, 3), (3, 3), (2, 3)] + top[3:]]
    recs = []
    for roads in (straight, merge):
        cells = np.asarray([p[0] * L + p[1] for r in roads for p in r], dtype=np.int32)
        off = np.cumsum([0] + [len(r) for r in roads]).astype(np.int32)
        rec = np.zeros(8 + L * L, np.uint32)
        assert _lib.lib.td_layout_from_roads(L, len(roads), _lib.ptr(cells, _lib.ctypes.c_int32),
                                             _lib.ptr(off, _lib.ctypes.c_int32), _lib.ptr(rec, _lib.ctypes.c_uint32)) == 0
        recs.append(rec)
    return recs


def reset_ok(env):
    """reset(), redrawing from the same stream the layouts whose road generation fails (as
    the device's auto-reset skips them)."""
    while True:
        try:
            return env.reset()
        except O.RoadGenError:
            pass


def oracle_state(env):
    st = canon.oracle_state(env)
    st["num_roads"] = env.num_roads
    return st


def pick_def(rng, mask, n_cells):
    """Index into the flat defender mask (6 * n_cells entries, + the no-op when discrete), or
    -1 for "nothing": with probability 0.3, or when nothing else is legal, nothing; else
    with probability 0.9 a legal non-destruct action if there is one; else any legal one."""
    legal = np.flatnonzero(mask.reshape(-1)[:6 * n_cells])
    if rng.random_sample() < 0.3 or len(legal) == 0:
        return -1
    keep = legal[legal < 5 * n_cells]
    if rng.random_sample() < 0.9 and len(keep):
        return int(keep[rng.randint(len(keep))])
    return int(legal[rng.randint(len(legal))])


def def_action(k, L, multi):
    """The env action of pick_def's index k."""
    if multi:
        a = np.zeros((6, L, L), dtype=np.int64)
        if k >= 0:
            a.reshape(-1)[k] = 1
        return a
    return 6 * L * L if k < 0 else k


def pick_atk(rng, mask):
    """(road, type) of one legal summon, or None: with probability 0.3, or when there is none."""
    legal = np.argwhere(mask[:, :4] != 0)
    if rng.random_sample() < 0.3 or len(legal) == 0:
        return None
    r, t = legal[rng.randint(len(legal))]
    return int(r), int(t)


def atk_action(rt):
    a = np.full((3, 8), 4, dtype=np.int64)
    if rt is not None:
        a[rt[0], 0] = rt[1]
    return a
