"""Shared pieces of the frame-skip tests (tests/test_frame_skip_ref.py on the CPU oracles,
tests/test_gpu_frame_skip.py on the device): the reference recipe and one board's reference
macro step.  Not a test module.

The reference of a macro step of k is the env stepped sub-step by sub-step -- the action, then
the empty action -- stopped at ``done`` and reset with the board's next layout draw that
succeeds, the rewards summed left to right in f64.  Observation, reward, done and state come
from the C restatement (oracle.td_cpu.Env); the info fields it does not return (RealAction,
FailCode, Win, AllowNextMove, the cool-downs) from the Python oracle (oracle.td_oracle.Env)
stepped beside it with the same actions."""
import numpy as np

from oracle import td_cpu as C
from oracle import td_oracle as O

ROAD_ATTEMPTS = 1000  # td_kernels.h kRoadAttempts
LAYOUT_RETRIES = 64   # td_kernels.h kLayoutRetries
MODES = {"def": O.MODE_DEF, "atk": O.MODE_ATK, "2p": O.MODE_2P}

# The recipe: one base life point and a fast attacker, so that episodes end every few dozen
# board steps, 40 boards of 10x10 from seed 500, board b shifted by b % k single empty steps,
# then 60 macro steps of uniform random actions from RandomState(1).
RECIPE = dict(base_LP=1, attacker_cost_init_rate=4, attacker_cost_final_rate=8)
RECIPE_BOARDS, RECIPE_STEPS, RECIPE_SEED0 = 40, 60, 500
# (mode, k): the even k are left out for TD-atk / TD-2p, whose episodes under this recipe end
# almost only at odd sub-step positions
RECIPE_CASES = [("def", 2), ("def", 3), ("def", 4), ("def", 8), ("atk", 3), ("2p", 3)]


def recipe_cfg(**over):
    return O.Config(**dict(RECIPE, **over))


class Ref(object):
    """One board's reference.  ``info``: step the Python oracle too (the info fields);
    ``c_env``: step the C restatement (False with ``hp``, which it does not take)."""

    def __init__(self, L, mode, seed, cfg, info=True, c_env=True, hp=None):
        self.L, self.mode = L, mode
        self.c = C.Env(L, mode, 1, seed, seed, cfg, road_attempts=ROAD_ATTEMPTS) if c_env else None
        try:
            self.o = O.Env(L, MODES[mode], 1, seed, seed, cfg, hp, road_attempts=ROAD_ATTEMPTS) if info else None
        except O.RoadGenError:
            if self.c is None:
                raise
            raise AssertionError("the two oracles disagree on seed %d" % seed)
        self.ep_ret = 0.0
        self.ep_len = 0
        self.empty_def = 6 * L * L
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
        d0 = self.empty_def if def_act is None else int(def_act)
        a0 = self.empty_atk if atk_act is None else np.asarray(atk_act, dtype=np.int64).reshape(3, 8)
        out = {}
        total = 0.0
        for j in range(k):
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
        if done:  # the device returns the next episode's first observation
            ob = self._reset()
            self.ep_ret, self.ep_len = 0.0, 0
        out["obs"] = ob
        return out

    def _actions_info(self, info, d0, a0):
        """real_def / fail_def / real_atk [3, 8] / fail_atk [3] (-1: no entry) as td_step_io has them."""
        out = {}
        real, fc = info["RealAction"], info["FailCode"]
        if self.mode == "def":
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


def make_refs(L, n, mode, cfg, seed0=RECIPE_SEED0, info=True, c_env=True, hp=None):
    """The first n seeds from seed0 whose first layout draw succeeds, with their references."""
    seeds, refs = [], []
    s = seed0
    while len(seeds) < n:
        try:
            refs.append(Ref(L, mode, s, cfg, info=info, c_env=c_env, hp=hp))
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
