"""The device against the oracle under fuzzed game configs (tests/cfgspace.py): every double of
the config with a full mantissa, the integer fields at their edges, the edge values of the rule
arithmetic planted.  Every board at every step through steputil.check_board -- reward bits, done,
state digest, all 45 x L x L observation bytes, win, cool-downs, AllowNextMove, RealAction /
FailCode -- with the engine's retained observation on (the oracle's full observation is the
expectation), and td_action_mask against the oracle-side mask on every fifth step.

Twelve cases (tests/test_config_space_ref.py runs the same ones on the two CPU oracles and counts
what they reach), each L = 10 case on the large kernel and on one of the small ones; further runs
with a float16 observation, at frame skip 3, with partial steps (td_step_boards) and with a
switch to a second fuzzed config in the middle.  And the config boundary: what the device cannot
represent is refused, with nothing changed."""
import copy
import math

import numpy as np
import pytest
import torch

import cfgspace as S
import handmaps
import maskutil as M
import steputil
from oracle import canon
from oracle import td_oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import params as P  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402
from gym_TD.masks import reference_masks  # noqa: E402

RUNS = [(c.name, k, "plain") for c in S.CASES for k in c.kernels] + \
       [(c.name, c.kernels[-1], v) for c in S.CASES for v in c.variants]


def _engine(case, cfg, seeds, kernel, **kw):
    eng = TDEngine(case.L, case.B, case.mode, case.multi, case.difficulty, np_seeds=seeds, py_seeds=seeds,
                   autoreset=False, cfg=cfg, hp=case.hyper(), step_kernel=kernel, **kw)
    if case.L == 7:  # caller layouts: create_road_v2 cannot draw a 7x7 map
        recs = [handmaps.record(r, 7) for r in S.ROADS7]
        eng.reset_layouts(np.stack([recs[b % 2] for b in range(case.B)]), np.arange(case.B))
    else:
        _, failed = eng.reset()
        assert not failed
    return eng


def _macro(o, k, d, a):
    """k board steps of oracle env ``o`` as one macro step (skiputil.Ref.macro's rule): the action,
    then empty actions, stopped at done; the rewards summed left to right; RealAction / FailCode
    of the first board step, everything else of the last."""
    total, first = 0.0, None
    for j in range(k):
        ob, r, done, info = o.step(d if j == 0 else (o.empty_def() if d is not None else None),
                                   a if j == 0 else (o.empty_atk() if a is not None else None))
        total = r if j == 0 else total + r
        first = first or info
        if done:
            break
    out = dict(first, Win=info["Win"], AllowNextMove=info["AllowNextMove"])
    return ob, total, done, out


def _check_masks(eng, case, envs, live, where):
    m = {k: v.cpu().numpy() for k, v in eng.action_mask(code=True).items()}
    for b in live:
        o = envs[b]
        dm, dc, am = reference_masks(M.oracle_state(o), case.L, o.cfg, o.hp, case.mode, case.multi)
        if case.mode != "atk":
            assert np.array_equal(m["def"][b], dm) and np.array_equal(m["def_code"][b], dc), (where, b, "def mask")
        if case.mode != "def":
            assert np.array_equal(m["atk"][b], am), (where, b, "atk mask")


@pytest.mark.parametrize("name,kernel,variant", RUNS)
def test_fuzzed_config_vs_oracle(name, kernel, variant):
    case = S.CASE[name]
    cfg = case.cfg()
    seeds, envs = S.make_envs(case, cfg)
    f16, skip = variant == "f16", 3 if variant == "skip3" else 1
    eng = _engine(case, copy.deepcopy(cfg), seeds, kernel, obs_dtype=torch.float16 if f16 else torch.float32,
                  frame_skip=skip)
    try:
        assert eng.step_kernel == kernel and eng.retain_obs
        rng = np.random.RandomState(case.seed)
        part = np.random.RandomState(case.seed + 1)
        steps = case.steps // skip
        compared = 0
        prev = None
        for k in range(steps):
            if variant == "switch" and k == S.SWITCH_AT:
                ov = S.switch_overrides(case)
                for key, v in ov.items():  # the envs share ``cfg``; live enemies and towers keep what they captured
                    setattr(cfg, key, copy.deepcopy(v))
                ep = _lib.lib.td_config_epoch(eng._h)
                eng.set_config(copy.deepcopy(cfg), case.hyper())
                assert _lib.lib.td_config_epoch(eng._h) != ep
            live = [b for b, o in enumerate(envs) if not o._board.done()]  # (no auto-reset: a finished board stays out)
            if k % 5 == 0:
                _check_masks(eng, case, envs, live, (name, k))
            da, aa = S.draw_actions(case, rng, envs)
            td = None if da is None else torch.from_numpy(da)
            ta = None if aa is None else torch.from_numpy(aa)
            idle = []
            if variant == "partial" and k % 3 == 2:
                ids = np.flatnonzero(part.random_sample(case.B) < 0.4)
                eng.step_boards(ids, def_act=td, atk_act=ta)
                idle = [b for b in live if b not in set(ids.tolist())]
                live = [b for b in live if b in set(ids.tolist())]
            else:
                eng.step(def_act=td, atk_act=ta)
            out = steputil.outputs(eng)
            for b in idle:  # a board the partial step did not name: its state and its output rows as they were
                where = (name, kernel, variant, k, b, "not named")
                assert canon.state_digest(eng.board_state(b, out["state"])) == canon.state_digest(canon.oracle_state(envs[b])), where
                for key in ("obs", "reward", "done", "win", "allow_next", "cooldowns", "real_def", "fail_def", "real_atk", "fail_atk"):
                    if out[key] is not None:
                        assert np.array_equal(out[key][b], prev[key][b]), where + (key,)
            prev = out
            for b in live:
                o = envs[b]
                d, a = S.act_of(case, da, aa, b)
                stepped = o.step(d, a) if skip == 1 else _macro(o, skip, d, a)
                want = S.pad_obs(stepped[0])
                steputil.check_board(eng, out, b, o, stepped, case.mode, case.multi, (name, kernel, variant, k, b),
                                     want_obs=want.astype(np.float16) if f16 else want)
                compared += 1
        # the oracle's own reach, fixed by the seeds: a case that came to end its boards early would compare little
        assert compared >= case.reach * case.B * steps * (0.88 if variant == "partial" else 1.0), compared
        assert (eng.flags() == 0).all()
    finally:
        eng.close()


# ---------------------------------------------------------------------------- the boundary
_REFUSED = [("frozen_time", 2.5), ("base_LP", 4.5), ("tower_distance", 1.5), ("attacker_action_interval", 1.25),
            ("defender_action_interval", 16.5), ("attacker_action_interval", -1), ("defender_action_interval", -2),
            ("reward_time", math.nan), ("frozen_ratio", math.inf), ("max_cost", -math.inf),
            ("tower_attack", [[454, 540], [651, math.nan], [566, 691], [358, 424]])]


@pytest.mark.parametrize("field,value", _REFUSED, ids=["%s=%r" % (f, v if not isinstance(v, list) else "nan") for f, v in _REFUSED])
def test_unrepresentable_config_is_refused(field, value):
    """td_create and td_set_config refuse a fraction in an integer-typed field, a negative
    interval and a NaN / infinity anywhere -- TDError, the field named.  A refused set_config
    leaves the config epoch and the retained observation as they were: the engine goes on
    stepping bit-exactly under its old config, skipping clean windows as before."""
    case = S.CASE["bal-def"]
    cfg = case.cfg()
    bad = copy.deepcopy(cfg)
    setattr(bad, field, value)
    with pytest.raises(_lib.TDError, match=field):
        TDEngine(case.L, 4, case.mode, cfg=bad, hp=case.hyper())
    seeds, envs = S.make_envs(case, cfg)
    eng = _engine(case, copy.deepcopy(cfg), seeds, "large")
    try:
        rng = np.random.RandomState(3)
        for k in range(24):
            if k == 12:
                ep, kept = _lib.lib.td_config_epoch(eng._h), _lib.lib.td_retained_obs(eng._h)
                assert kept == eng.obs.data_ptr()
                with pytest.raises(_lib.TDError, match=field):
                    eng.set_config(bad, case.hyper())
                assert _lib.lib.td_config_epoch(eng._h) == ep and _lib.lib.td_retained_obs(eng._h) == kept
            da, aa = S.draw_actions(case, rng, envs)
            eng.step(def_act=torch.from_numpy(da))
            out = steputil.outputs(eng)
            for b, o in enumerate(envs):
                stepped = o.step(*S.act_of(case, da, aa, b))
                steputil.check_board(eng, out, b, o, stepped, case.mode, False, (field, k, b), want_obs=S.pad_obs(stepped[0]))
    finally:
        eng.close()


def test_tower_distance_may_not_grow_under_standing_towers():
    """The reference subtracts a destructed tower's diamond at the current tower_distance: after
    paramConfig(tower_distance=larger) it takes map[6] below zero, and to zero under another
    tower, where a second tower may then be built on the same cell.  The device's cell word has
    an unsigned count and room for one tower, so td_set_config refuses a larger tower_distance
    while any board holds a tower -- nothing changed -- and takes it once none does; a smaller
    one is always taken."""
    case = S.CASE["fort-def"]
    cfg = case.cfg()
    seeds, envs = S.make_envs(case, cfg)
    eng = _engine(case, copy.deepcopy(cfg), seeds, "large")
    try:
        wider, narrower = copy.deepcopy(cfg), copy.deepcopy(cfg)
        wider.tower_distance, narrower.tower_distance = cfg.tower_distance + 1, cfg.tower_distance - 1
        assert narrower.tower_distance >= 0
        ep = _lib.lib.td_config_epoch(eng._h)
        eng.set_config(wider, case.hyper())  # no tower yet
        eng.set_config(copy.deepcopy(cfg), case.hyper())
        assert _lib.lib.td_config_epoch(eng._h) != ep
        rng = np.random.RandomState(1)
        while not int(eng.export_state()["hdr"]["n_tw"].max()):
            da, _ = S.draw_actions(case, rng, envs)
            eng.step(def_act=torch.from_numpy(da))
            for b, o in enumerate(envs):
                o.step(int(da[b]))
        ep, kept = _lib.lib.td_config_epoch(eng._h), _lib.lib.td_retained_obs(eng._h)
        with pytest.raises(_lib.TDError, match="tower_distance may not grow"):
            eng.set_config(wider, case.hyper())
        assert _lib.lib.td_config_epoch(eng._h) == ep and _lib.lib.td_retained_obs(eng._h) == kept
        da, aa = S.draw_actions(case, rng, envs)  # the engine goes on under its old config
        eng.step(def_act=torch.from_numpy(da))
        out = steputil.outputs(eng)
        for b, o in enumerate(envs):
            stepped = o.step(int(da[b]))
            steputil.check_board(eng, out, b, o, stepped, case.mode, False, ("after the refusal", b), want_obs=S.pad_obs(stepped[0]))
        eng.set_config(narrower, case.hyper())
        assert _lib.lib.td_config_epoch(eng._h) != ep
    finally:
        eng.close()


def test_paramconfig_refusal_keeps_the_config():
    """gym_TD.paramConfig with a live engine: the refusal is a TDError and gym_TD.params.config
    keeps its value; the next paramConfig goes through."""
    import gym_TD
    old = P.config.frozen_time
    eng = TDEngine(10, 2, "def")
    try:
        with pytest.raises(_lib.TDError, match="frozen_time"):
            gym_TD.paramConfig(frozen_time=2.5)
        assert P.config.frozen_time == old
        ep = _lib.lib.td_config_epoch(eng._h)
        gym_TD.paramConfig(frozen_time=3)
        assert _lib.lib.td_config_epoch(eng._h) != ep
    finally:
        eng.close()
        gym_TD.paramConfig(frozen_time=old)
