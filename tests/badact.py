"""Out-of-range actions (TD_FLAG_BAD_ACTION): the device's rule restated, and reference runs
that send such actions.  Shared by tests/test_bad_action_ref.py (CPU: the runs reach what
they are meant to reach) and tests/test_gpu_bad_action.py (the device against them).  Not a
test module.

The rule (include/tdstep.h, td_board_flag): a discrete defender action outside 0 .. 6 L^2
becomes 6 L^2, the empty action; each attacker entry outside 0 .. 4 becomes 4, "none"; each
multi-action flag outside 0 .. 2 counts as 0; the board is flagged in that step, cooling down
or not, and the step runs exactly as with the sanitised action.  The reference asserts on
such input, so the oracles are stepped with the sanitised action: ``sanitise`` below is the
only rule code on the test side.

The values sent: -1, -2^63, 2^31, one past the space, and 2^32 + a with a legal ``a`` that
would change the board right now -- a kernel that looks at the low word only acts on ``a``.
"""
import pickle

import numpy as np

import maskutil as M
import skiputil as S
from gym_TD.masks import reference_masks
from oracle import canon

FLAG_BAD_ACTION = 4  # include/tdstep.h td_board_flag
B, STEPS, SEED0 = 16, 40, 500
KINDS = ("minus1", "min", "2^31", "past", "hi")
HI = 1 << 32
# on top of the frame-skip recipe: the action intervals (both sides cool down), enemies fast
# enough to end episodes within 40 single steps on 20x20 roads too, and a defender with an
# income, so that an affordable build -- a live ``a`` -- exists at most steps
COOL = dict(enemy_speed=[[.9, .9], [.7, .7], [.6, .6], [.6, .6]], defender_init_cost=60, defender_cost_rate=2.0)


def sanitise(L, d=None, a=None, multi=False):
    """(defender action, attacker action, any value out of range) as the device takes them."""
    bad = False
    if d is not None:
        if multi:
            d = np.asarray(d, dtype=np.int64)
            off = (d < 0) | (d > 2)
            bad, d = bool(off.any()), np.where(off, 0, d)
        elif d < 0 or d > 6 * L * L:
            bad, d = True, 6 * L * L
    if a is not None:
        a = np.asarray(a, dtype=np.int64)
        off = (a < 0) | (a > 4)
        bad, a = bad or bool(off.any()), np.where(off, 4, a)
    return d, a, bad


def _value(kind, past, a):
    return {"minus1": -1, "min": -2 ** 63, "2^31": 2 ** 31, "past": past, "hi": HI + a}[kind]


def _clone(env):
    return pickle.loads(pickle.dumps(env, pickle.HIGHEST_PROTOCOL))


def _after(env, d, a, k=1):
    """(state digest, sub-step at which the episode ended or -1) of a copy of the Python oracle
    stepped with (d, a), then k - 1 empty actions."""
    e = _clone(env)
    for j in range(k):
        done = e.step(d if j == 0 or d is None else e.empty_def(), a if j == 0 or a is None else e.empty_atk())[2]
        if done:
            return canon.state_digest(canon.oracle_state(e)), j
    return canon.state_digest(canon.oracle_state(e)), -1


class Trace(object):
    """One reference run: B boards, STEPS (macro) steps, auto-reset, the frame-skip recipe
    with action intervals of 3 (defender) and 2 (attacker) -- 5 and 4 at frame skip 3.

    Actions are legal ones from RandomState(rng): mask-driven picks (maskutil.pick_def /
    pick_atk: about 70 % of the steps act, so both sides do cool down), random multi-action
    flags in {0, 1, 2}.  Odd boards never get a bad value.  Even board b gets one at the
    steps s >= b // 2 with (s + b) % 3 == 0, and at every step that ends its episode with the
    empty action (looked ahead on a copy of the oracle), so that flags are set in the very
    step that auto-resets the board.  The kinds rotate per board; when the side is off
    cool-down and the mask has a legal ``a``, two in three are 2^32 + a, the rest of that
    side's action empty so that ``a`` alone decides.  TD-2p alternates the side, both sides
    in every third.

    Per step: ``acts`` (def, atk as sent), ``outs`` (skiputil.Ref.macro of the sanitised
    actions plus "digest", the state digest), ``flags`` (each board's expected flag word).
    Counted: ``live`` (2^32 + a cases where stepping a copy of the oracle with ``a`` gives
    another state digest than the sanitised action does), ``cool`` (bad values sent to a side
    that is cooling down), ``kinds``, ``ends_bad`` [k] (macro steps that carried a bad value
    and ended the episode at sub-step j), ``both`` (TD-2p: both sides bad in one step)."""

    def __init__(self, mode, L, multi=False, k=1, rng=11):
        self.mode, self.L, self.multi, self.k = mode, L, multi, k
        # action intervals of 3 and 2; at frame skip 3 those have always run out by the next
        # macro step's sub-step 0, the only one that takes an action: 5 and 4 there
        di, ai = (3, 2) if k == 1 else (5, 4)
        self.cfg = S.recipe_cfg(defender_action_interval=di, attacker_action_interval=ai, **COOL)
        self.seeds, refs = S.make_refs(L, B, mode, self.cfg, seed0=SEED0, multi=multi)
        self.rng = np.random.RandomState(rng)
        self.live = self.cool = self.both = 0
        self.kinds = dict.fromkeys(KINDS, 0)
        self.ends_bad = [0] * k
        self.acts, self.outs, self.flags = [], [], []
        self._n = [0] * B
        flag = np.zeros(B, dtype=np.int32)
        try:
            self.first = [r.obs() for r in refs]
            for s in range(STEPS):
                d_all = [] if mode != "atk" else None
                a_all = [] if mode != "def" else None
                row = []
                for b, ref in enumerate(refs):
                    d, a = self._legal(ref.o)
                    if b % 2 == 0:
                        hit = s >= b // 2 and (s + b) % 3 == 0
                        ed = None if d is None else ref.empty_def
                        ea = None if a is None else ref.empty_atk
                        if hit or _after(ref.o, ed, ea, k)[1] >= 0:
                            d, a = self._inject(ref.o, b, d, a)
                    sd, sa, bad = sanitise(L, d, a, multi)
                    if bad:
                        flag[b] |= FLAG_BAD_ACTION
                    out = ref.macro(k, sd, sa)
                    out["digest"] = canon.digest(ref.state_bytes())
                    if bad and out["done"]:
                        self.ends_bad[out["ran"] - 1] += 1
                    row.append(out)
                    if d_all is not None:
                        d_all.append(d)
                    if a_all is not None:
                        a_all.append(a)
                self.acts.append((None if d_all is None else np.asarray(d_all, dtype=np.int64),
                                  None if a_all is None else np.asarray(a_all, dtype=np.int64)))
                self.outs.append(row)
                self.flags.append(flag.copy())
        finally:
            for r in refs:
                r.close()
        self.resets_flagged = sum(1 for s in range(STEPS - 1) for b in range(B)
                                  if self.outs[s][b]["done"] and self.flags[s][b] and s + 1 < STEPS)

    # ---- legal actions
    def _masks(self, o):
        return reference_masks(M.oracle_state(o), self.L, o.cfg, o.hp, self.mode, self.multi, cap=False)

    def _legal(self, o):
        rng, L = self.rng, self.L
        dm, _, am = self._masks(o)
        d = a = None
        if self.mode != "atk":
            pick = M.pick_def(rng, dm, L * L)
            if self.multi:  # the picked flag among sparse random ones and 2s (2 means nothing)
                d = M.def_action(pick, L, True)
                d |= (rng.random_sample((6, L, L)) < 0.02).astype(np.int64)
                d[rng.random_sample((6, L, L)) < 0.05] = 2
            else:
                d = int(M.def_action(pick, L, False)) if rng.random_sample() < 0.8 else int(rng.randint(0, 6 * L * L + 1))
        if self.mode != "def":
            a = M.atk_action(M.pick_atk(rng, am))
            if rng.random_sample() < 0.3:
                a = rng.randint(0, 5, size=(3, 8)).astype(np.int64)
        return d, a

    # ---- bad values
    def _inject(self, o, b, d, a):
        """The step's actions with a bad value in them (both sides sometimes in TD-2p)."""
        n = self._n[b]
        self._n[b] += 1
        sides = {"def": "d", "atk": "a"}.get(self.mode) or ("da" if n % 3 == 2 else "d" if n % 3 == 0 else "a")
        if len(sides) == 2:
            self.both += 1
        low_d = low_a = None  # the action with the low word of a 2^32 + a value in its place
        for i, side in enumerate(sides):
            kind = KINDS[(n // 2 + b // 2 + i) % 4]
            cooling = (o.defender_cd if side == "d" else o.attacker_cd) >= 2
            self.cool += cooling
            if side == "d":
                d, low_d = self._inject_def(o, d, kind, n % 3 != 0 and not cooling)
            else:
                a, low_a = self._inject_atk(o, a, kind, n % 3 != 0 and not cooling)
        # live: on a copy of the oracle, ``a`` in place of 2^32 + a (everything else as the
        # device takes it) leaves another state than the sanitised action does
        sd, sa, _ = sanitise(self.L, d, a, self.multi)
        if low_d is not None:
            self.live += _after(o, low_d, sa)[0] != _after(o, sd, sa)[0]
        if low_a is not None:
            self.live += _after(o, sd, low_a)[0] != _after(o, sd, sa)[0]
        return d, a

    def _inject_def(self, o, d, kind, want_hi):
        """(the defender action with a bad value, its low-word twin if that is 2^32 + a)."""
        L, rng = self.L, self.rng
        legal = np.flatnonzero(self._masks(o)[0].reshape(-1)[:5 * L * L])  # builds and upgrades
        if want_hi and len(legal):
            kind, k = "hi", int(legal[rng.randint(len(legal))])
        else:
            k = int(rng.randint(0, 6 * L * L))
        self.kinds[kind] += 1
        if self.multi:
            if kind == "hi":
                d = np.zeros((6, L, L), dtype=np.int64)
                d.reshape(-1)[k] = HI + 1
                return d, M.def_action(k, L, True)
            else:
                d = d.copy()
                d.reshape(-1)[k] = _value(kind, 3, 0)
                if rng.random_sample() < 0.5:  # and a second one, at the other end of a 16-B unit
                    d.reshape(-1)[k ^ 1] = _value(kind, 3, 0)
            return d, None
        return _value(kind, 6 * L * L + 1, k), (k if kind == "hi" else None)

    def _inject_atk(self, o, a, kind, want_hi):
        """(the attacker action with bad values, its low-word twin if that is 2^32 + a)."""
        rng = self.rng
        am = self._masks(o)[2]
        legal = np.argwhere(am[:, :4] != 0)
        if want_hi and len(legal):
            r, t = legal[rng.randint(len(legal))]
            slot = int(rng.randint(8))
            self.kinds["hi"] += 1
            a = np.full((3, 8), 4, dtype=np.int64)
            a[r, slot] = HI + int(t)
            low = np.full((3, 8), 4, dtype=np.int64)
            low[r, slot] = int(t)
            return a, low
        self.kinds[kind] += 1
        a = a.copy()
        r, slot = int(rng.randint(3)), int(rng.randint(8))
        a[r, slot] = _value(kind, 5, 0)
        a[r, (slot + 3) % 8] = _value(kind, 5, 0)  # two entries of one cluster: each becomes 4
        return a, None


# the cases: (mode, multi, L); the kernels and observation formats each runs on are the GPU test's
DISCRETE = [(m, False, L) for m in ("def", "atk", "2p") for L in (10, 20, 12)]
MULTI = [(m, True, L) for m in ("def", "2p") for L in (10, 20, 11)]
SKIP = [(m, False, L) for m in ("def", "atk", "2p") for L in (10, 11)]  # at frame skip 3
SKIP_K = 3

_cache = {}


def trace(mode, multi, L, k=1):
    """The case's Trace, computed once and shared (the last two are kept: the tests of one
    case on its kernels and formats run back to back)."""
    key = (mode, multi, L, k)
    if key not in _cache:
        if len(_cache) >= 2:
            _cache.clear()
        _cache[key] = Trace(mode, L, multi, k)
    return _cache[key]


def check_trace(tr):
    """What a run has to reach by itself, on the CPU (raises AssertionError)."""
    what = (tr.mode, tr.multi, tr.L, tr.k, tr.live, tr.cool, tr.kinds, tr.ends_bad, tr.both, tr.resets_flagged)
    assert tr.live >= 8, what  # 2^32 + a cases whose ``a`` would have changed the board
    assert tr.cool >= 4, what  # bad values sent to a side that is cooling down
    assert all(n >= 1 for n in tr.kinds.values()), what
    last = tr.flags[-1]
    assert (last[1::2] == 0).all() and (last[0::2] == FLAG_BAD_ACTION).all(), what
    late = [next(s for s in range(STEPS) if tr.flags[s][b]) for b in range(0, B, 2)]
    assert max(late) >= 4, what  # boards flagged late: "not one step earlier" is checked on them
    assert tr.resets_flagged >= 1, what  # a flag carried across an auto-reset
    assert sum(tr.ends_bad) >= 1, what  # a flag set in the step that auto-resets the board
    if tr.mode == "2p":
        assert tr.both >= 4, what
    if tr.k > 1:  # the bad value's macro step ends the episode at each sub-step position
        assert all(n >= 1 for n in tr.ends_bad), what
