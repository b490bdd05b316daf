"""Shared pieces of the frame-skip tests (tests/test_frame_skip_ref.py on the CPU oracles,
tests/test_gpu_frame_skip.py on the device): the reference recipe, one board's reference
macro step (used by tests/badact.py too) and the run that changes the config before every
macro step.  Not a test module.

The reference of a macro step of k is the env stepped sub-step by sub-step -- the action, then
the empty action -- stopped at ``done`` and reset with the board's next layout draw that
succeeds, the rewards summed left to right in f64.  Observation, reward, done and state come
from the C restatement (oracle.td_cpu.Env); the info fields it does not return (RealAction,
FailCode, Win, AllowNextMove, the cool-downs) from the Python oracle (oracle.td_oracle.Env)
stepped beside it with the same actions."""
import contextlib
import copy

import numpy as np

from oracle import policies
from oracle import td_cpu as C
from oracle import canon
from oracle import td_oracle as O

ROAD_ATTEMPTS = 1000  # td_kernels.h kRoadAttempts
LAYOUT_RETRIES = 64   # td_kernels.h kLayoutRetries
MODES = {"def": O.MODE_DEF, "atk": O.MODE_ATK, "2p": O.MODE_2P}

# The recipe: one base life point and a fast attacker, so that episodes end every few dozen
# board steps, 40 boards of 10x10 from seed 500, board b shifted by b % k single empty steps,
# then 60 macro steps of uniform random actions from RandomState(1).
RECIPE = dict(base_LP=1, attacker_cost_init_rate=4, attacker_cost_final_rate=8)
RECIPE_BOARDS, RECIPE_STEPS, RECIPE_SEED0 = 40, 60, 500
# (mode, k).  TD-def ends episodes at every sub-step position, up to k = 16, the maximum.  The
# episodes of TD-atk / TD-2p end unevenly under this recipe at even k (at k = 4 never at
# position 2): those cases have floors of their own, see check_ends.
RECIPE_CASES = [("def", 2), ("def", 3), ("def", 4), ("def", 8), ("def", 16), ("atk", 3), ("2p", 3),
                ("atk", 4), ("2p", 4), ("atk", 16), ("2p", 16)]
ENDS_FLOOR = 5


def recipe_steps(mode, k):
    """Macro steps of a recipe case: 60, but 30 for TD-atk / TD-2p at k = 16."""
    return 30 if mode != "def" and k == 16 else RECIPE_STEPS


def check_ends(mode, k, ends):
    """The floors on the episode ends per sub-step position (``ends`` [k]) of a recipe case,
    all below what the Python oracle alone gave: at least 5 at every position; TD-atk / TD-2p
    at k = 4 (measured [5, 7, 0, 98] and [3, 9, 0, 104]) at least 3 at positions 0, 1 and 3,
    and at k = 16 (165 and 205 ends over 13 positions each) at least 100 ends over at least
    10 distinct positions."""
    ends = np.asarray(ends)
    assert len(ends) == k, (mode, k, ends.tolist())
    if mode != "def" and k == 4:
        assert (ends[[0, 1, 3]] >= 3).all(), (mode, k, ends.tolist())
    elif mode != "def" and k == 16:
        assert ends.sum() >= 100 and np.count_nonzero(ends) >= 10, (mode, k, ends.tolist())
    else:
        assert (ends >= ENDS_FLOOR).all(), (mode, k, ends.tolist())


def recipe_cfg(**over):
    return O.Config(**dict(RECIPE, **over))


class Ref(object):
    """One board's reference.  ``info``: step the Python oracle too (the info fields);
    ``c_env``: step the C restatement (False with ``hp``, which it does not take);
    ``multi``: multi-action defender flags (6, L, L) (frame skip 1 only on the device).
    ``autoreset`` (attribute, default True): False leaves a finished board finished."""
    autoreset = True

    def __init__(self, L, mode, seed, cfg, info=True, c_env=True, hp=None, multi=False):
        self.L, self.mode, self.multi = L, mode, multi
        if multi and hp is None:
            hp = O.Hyper(allow_multiple_actions=True)
        self.c = C.Env(L, mode, 1, seed, seed, cfg, multi=multi, road_attempts=ROAD_ATTEMPTS) if c_env else None
        try:
            self.o = O.Env(L, MODES[mode], 1, seed, seed, cfg, hp, road_attempts=ROAD_ATTEMPTS) if info else None
        except O.RoadGenError:
            if self.c is None:
                raise
            raise AssertionError("the two oracles disagree on seed %d" % seed)
        self.ep_ret = 0.0
        self.ep_len = 0
        self.empty_def = np.zeros((6, L, L), dtype=np.int64) if multi else 6 * L * L
        self.empty_atk = np.full((3, 8), 4, dtype=np.int64)

    def close(self):
        if self.c is not None:
            self.c.close()

    def obs(self):
        return self.c.obs() if self.c is not None else self.o._board.get_states()

    def state_bytes(self):
        return self.c.state_bytes()

    def _reset(self):
        """Auto-reset's layout: the next draw that succeeds (failing draws skipped)."""
        ob = None
        for env, err in ((self.c, C.RoadGenError), (self.o, O.RoadGenError)):
            if env is None:
                continue
            for _ in range(LAYOUT_RETRIES + 1):
                try:
                    got = env.reset()
                    break
                except err:
                    pass
            else:
                raise AssertionError("no layout in %d draws" % (LAYOUT_RETRIES + 1))
            ob = got if ob is None else ob
        return ob

    def _one(self, d, a):
        info = None
        if self.c is not None:
            ob, r, done = self.c.step(d if self.mode != "atk" else None, a if self.mode != "def" else None)
        if self.o is not None:
            po, pr, pdone, info = self.o.step(d if self.mode != "atk" else None, a if self.mode != "def" else None)
            if self.c is None:
                ob, r, done = po, pr, pdone
            else:  # the two oracles are pinned to each other elsewhere; a cheap guard here
                assert r.hex() == float(pr).hex() and done == pdone
        return ob, float(r), bool(done), info

    def macro(self, k, def_act=None, atk_act=None):
        """Up to k sub-steps; returns a dict of what one td_step at frame skip k must give."""
        d0 = self.empty_def if def_act is None else np.asarray(def_act, dtype=np.int64) if self.multi else int(def_act)
        a0 = self.empty_atk if atk_act is None else np.asarray(atk_act, dtype=np.int64).reshape(3, 8)
        out = {}
        total = 0.0
        for j in range(k):
            self.sub = j  # (the sub-step being run, for counting_late_summons)
            ob, r, done, info = self._one(d0 if j == 0 else self.empty_def, a0 if j == 0 else self.empty_atk)
            self.ep_ret = self.ep_ret + r  # dadd(ep_ret, r)
            self.ep_len += 1
            total = r if j == 0 else total + r  # r0, then left to right
            if j == 0 and info is not None:
                out.update(self._actions_info(info, d0, a0))
            if done:
                break
        out.update(reward=total, done=done, ran=j + 1, ep_ret=self.ep_ret, ep_len=self.ep_len)
        if info is not None:
            o = self.o
            w = info["Win"]
            if isinstance(w, dict):
                w = w["Defender"]
            out["win"] = -1 if w is None else int(bool(w))
            out["allow"] = (1 if o.attacker_cd <= 1 else 0) | (2 if o.defender_cd <= 1 else 0)
            out["cool"] = min(o.attacker_cd, 15) | (min(o.defender_cd, 15) << 4)
            assert o._board.steps == self.ep_len
        if done and self.autoreset:  # the device returns the next episode's first observation
            ob = self._reset()
            self.ep_ret, self.ep_len = 0.0, 0
        out["obs"] = ob
        return out

    def _actions_info(self, info, d0, a0):
        """real_def / fail_def / real_atk [3, 8] / fail_atk [3] (-1: no entry) as td_step_io has them."""
        out = {}
        real, fc = info["RealAction"], info["FailCode"]
        if self.multi:  # the real-action planes; the reference has no FailCode here
            if self.mode == "def":
                out["real_def"] = np.asarray(real, dtype=np.int64)
            else:
                out["real_def"] = np.asarray(real["Defender"], dtype=np.int64)
                out["real_atk"] = np.asarray(real["Attacker"], dtype=np.int64).reshape(3, 8)
        elif self.mode == "def":
            out["real_def"], out["fail_def"] = int(real), int(fc)
        elif self.mode == "atk":
            out["real_atk"] = np.asarray(real, dtype=np.int64).reshape(3, 8)
            out["fail_atk"] = np.asarray(list(fc) + [-1] * (3 - len(fc)), dtype=np.int32)
        else:
            # TDMulti.py:257 replaces the whole RealAction dict by the defender's action when it acted
            out["real_def"] = int(real["Defender"]) if isinstance(real, dict) else int(real)
            out["real_atk"] = a0.copy()
            out["fail_def"] = int(fc["Defender"])
            fa = fc["Attacker"]
            out["fail_atk"] = np.asarray(list(fa) + [-1] * (3 - len(fa)), dtype=np.int32)
        return out


def make_refs(L, n, mode, cfg, seed0=RECIPE_SEED0, info=True, c_env=True, hp=None, multi=False):
    """The first n seeds from seed0 whose first layout draw succeeds, with their references."""
    seeds, refs = [], []
    s = seed0
    while len(seeds) < n:
        try:
            refs.append(Ref(L, mode, s, cfg, info=info, c_env=c_env, hp=hp, multi=multi))
            seeds.append(s)
        except (C.RoadGenError, O.RoadGenError):
            pass
        s += 1
    return seeds, refs


def draw_actions(rng, mode, n, L):
    """Uniform random actions of one macro step: (def [n] or None, atk [n, 3, 8] or None)."""
    d = rng.randint(0, 6 * L * L + 1, size=n).astype(np.int64) if mode != "atk" else None
    a = rng.randint(0, 5, size=(n, 3, 8)).astype(np.int64) if mode != "def" else None
    return d, a


def act_of(acts, b):
    d, a = acts
    return (None if d is None else int(d[b])), (None if a is None else a[b])


# --------------------------------------------------------------------------
# td_set_config between macro steps
# --------------------------------------------------------------------------
# A cut-down tests/test_gpu_envs.py test_config_epochs_recycled_past_256 at frame skip 3: a new
# config before every macro step, on the engine and on every oracle's ``cfg``.  An enemy or tower
# keeps the values of the config it was created under, so the entities of sub-steps 1 and 2
# must capture the launch's config epoch like those of sub-step 0.
CFG_BASE = dict(tower_distance=0, defender_init_cost=150, max_cost=400, defender_cost_rate=0.5)
CFG_K, CFG_BOARDS, CFG_SEED0 = 3, 16, 6200


def cfg_at(i, into, base=CFG_BASE):
    """Config number i written into ``into`` (an oracle Config or a copy of gym_TD.params.config)."""
    for key, v in base.items():
        setattr(into, key, copy.deepcopy(v))
    into.reward_time = 0.001 + i * 1e-6  # every macro step's config is distinct
    into.enemy_LP = [[820 + 10 * (i % 11), 1700], [2050, 3000 + 7 * (i % 5)], [6000, 8000], [8000 - 3 * (i % 9), 12000]]
    into.enemy_defense = [[i % 3, 0], [200 + i % 7, 250], [600, 800], [80, 100]]
    into.enemy_speed = [[.25, .25], [.13 + .01 * (i % 2), .13], [.1, .1], [.1, .1]]
    into.tower_attack = [[454 + i % 13, 540], [651, 771 + i % 4], [566 + i % 6, 691], [358, 424]]
    into.tower_range = [[3 + i % 2, 3], [2, 2], [4, 4], [3, 3]]
    return into


@contextlib.contextmanager
def counting_late_summons(current, count):
    """Inside the block ``count[0]`` grows by the enemies that the Python oracle of
    ``current[0]`` (a Ref) summons in a sub-step >= 1."""
    summon0 = O.Board.summon_cluster

    def summon(board, types, road):
        ok, real = summon0(board, types, road)
        if current[0].sub >= 1:
            count[0] += sum(int(t) != board.cfg.enemy_types for t in real)
        return ok, real

    O.Board.summon_cluster = summon
    try:
        yield
    finally:
        O.Board.summon_cluster = summon0


class ConfigTrace(object):
    """TD-def, 10x10, 16 boards, frame skip 3, cfg_at(i) before macro step i, the discrete_def
    policy on RandomState(31), on the Python oracle (the C restatement takes its config once).
    ``autoreset`` False: 60 macro steps, a finished board stays finished (its later outs are
    None); True: 30 macro steps with RECIPE in CFG_BASE's place (the rich defender of CFG_BASE
    loses no episode), an episode that ends inside a macro step starts the next one under
    that launch's config.  Per macro step ``acts`` and ``outs`` (Ref.macro's
    dicts plus "digest"); ``late_summons``: enemies summoned in a sub-step >= 1;
    ``build_cfgs``: the configs under which a tower was built; ``ends``: episodes ended."""

    def __init__(self, autoreset):
        self.autoreset, self.k, self.L = autoreset, CFG_K, 10
        self.steps = 30 if autoreset else 60
        self.base = RECIPE if autoreset else CFG_BASE
        L, k = self.L, self.k
        self.seeds, refs = make_refs(L, CFG_BOARDS, "def", self.cfg(0, O.Config()), seed0=CFG_SEED0, c_env=False)
        self.first = [r.obs() for r in refs]
        rng = np.random.RandomState(31)
        self.acts, self.outs, self.build_cfgs, self.ends = [], [], set(), 0
        current, count = [None], [0]
        with counting_late_summons(current, count):
            for i in range(1, self.steps + 1):
                for ref in refs:
                    ref.autoreset = autoreset
                    self.cfg(i, ref.o.cfg)
                acts = np.array([policies.discrete_def(rng, L, r.o._board.map[0], 0.7) for r in refs], dtype=np.int64)
                row = []
                for b, ref in enumerate(refs):
                    if ref.o._board.done():  # (without auto-reset: finished in an earlier macro step)
                        row.append(None)
                        continue
                    current[0] = ref
                    out = ref.macro(k, int(acts[b]))
                    out["digest"] = canon.state_digest(canon.oracle_state(ref.o))
                    if out["real_def"] == int(acts[b]) and acts[b] < 4 * L * L:
                        self.build_cfgs.add(i)
                    self.ends += out["done"]
                    row.append(out)
                self.acts.append(acts)
                self.outs.append(row)
        self.late_summons = count[0]

    def cfg(self, i, into):
        return cfg_at(i, into, self.base)

    def check(self):
        """What the run is there for (raises AssertionError)."""
        what = (self.autoreset, self.late_summons, len(self.build_cfgs), self.ends)
        if self.autoreset:
            assert self.ends >= 5, what
        else:
            assert self.late_summons >= 20 and len(self.build_cfgs) >= 10, what
            assert sum(o is not None for o in self.outs[-1]) >= CFG_BOARDS // 2, what
