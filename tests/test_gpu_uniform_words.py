"""The step kernels' short cuts on a board's common path against the CPU oracle
(gym-td_amd/csrc/td_step_rules.h): the enemy level of a summon as an integer test on the step
count (td_upgrade_step.h), the cluster of eight equal types summoned by one loop, and the board
step that skips kills, march, leaks and compaction on a board without an enemy.

The cases are tests/uniformwords.py's (tests/test_uniform_words_ref.py runs them on the oracle
alone): 37 boards of 10x10 (xcd_board's remainder branch), auto-reset off, every board that still
runs compared after every step through steputil.check_board -- reward bits, done, state digest,
all 45 x L x L observation bytes, win, cool-downs, AllowNextMove, RealAction / FailCode -- with
the retained observation on.  A run is refused unless the oracle reached every event the case
names: clusters of which 0, 1 .. 7 and 8 slots succeed, a cost or a full list that stops a
cluster in the middle, fractions in enemy_cost, episodes that cross enemy_upgrade_at with prices
that differ by level (thresholds 0, 1.0 and 2.0 too), boards stepped past max_episode_steps,
callers' clusters of equal types, of 4s and mixed ones in TD-atk and TD-2p, boards that gain
their first enemy and lose their last, td_set_config in the middle of the episodes.  The one-wave,
two-wave and large kernels are forced; one run each writes a float16 observation, runs at frame
skip 3, and compares a retained engine with a retain_obs=False twin byte for byte."""
import copy

import numpy as np
import pytest
import torch

import steputil
import uniformwords as W

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD.engine import TDEngine  # noqa: E402

RUNS = [(c.name, k, "plain") for c in W.CASES for k in c.kernels] + \
       [(c.name, c.kernels[-1], v) for c in W.CASES for v in c.variants]
OUTPUTS = ("obs", "reward", "done", "win", "allow_next", "cooldowns", "ep_return", "ep_len", "real_def", "fail_def",
           "real_atk", "fail_atk")


def _engine(case, cfg, hp, seeds, kernel, **kw):
    eng = TDEngine(10, W.B, case.mode, case.multi, case.difficulty, np_seeds=seeds, py_seeds=seeds, autoreset=False,
                   cfg=copy.deepcopy(cfg), hp=copy.deepcopy(hp), step_kernel=kernel, **kw)
    _, failed = eng.reset()
    assert not failed
    assert eng.step_kernel == kernel
    return eng


def _same_bytes(a, b, where):
    for name in OUTPUTS:
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), name
        if ta is not None:
            assert torch.equal(ta.contiguous().view(torch.uint8), tb.contiguous().view(torch.uint8)), (name, where)


@pytest.mark.parametrize("name,kernel,variant", RUNS)
def test_case_vs_oracle(name, kernel, variant):
    case = W.CASE[name]
    seeds, envs, cfg, hp = W.make_envs(case)
    f16, skip = variant == "f16", 3 if variant == "skip3" else 1
    kw = dict(obs_dtype=torch.float16 if f16 else torch.float32, frame_skip=skip)
    eng = _engine(case, cfg, hp, seeds, kernel, **kw)
    twin = _engine(case, cfg, hp, seeds, kernel, retain_obs=False, **kw) if variant == "twin" else None
    led = W.Ledger()
    try:
        assert eng.retain_obs and (twin is None or not twin.retain_obs)
        rng = np.random.RandomState(case.rng)
        with W.counting(led):
            for k in range(case.steps // skip):
                if W.apply_switch(case, k, cfg, hp):
                    for e in (eng, twin):
                        if e is not None:
                            e.set_config(copy.deepcopy(cfg), copy.deepcopy(hp))
                run = W.live(case, envs)
                da, aa = W.draw_actions(case, rng, envs)
                td = None if da is None else torch.from_numpy(da)
                ta = None if aa is None else torch.from_numpy(aa)
                eng.step(def_act=td, atk_act=ta)
                if twin is not None:
                    twin.step(def_act=td, atk_act=ta)
                    _same_bytes(eng, twin, (name, k))
                out = steputil.outputs(eng)
                for b in run:
                    o = envs[b]
                    d, a = W.act_of(case, da, aa, b)
                    stepped = o.step(d, a) if skip == 1 else W.macro(o, skip, d, a)
                    steputil.check_board(eng, out, b, o, stepped, case.mode, case.multi, (name, kernel, variant, k, b),
                                         want_obs=stepped[0].astype(np.float16) if f16 else None)
        if skip == 1:  # (at frame skip the boards stop at the limit: the plain runs hold the floors)
            W.check_needs(case, led)
        assert len(W.live(case, envs)) >= W.B // 2, "most boards are compared to the end"
        want_flags = [1 if o.refused[0] else 0 for o in envs]  # TD_FLAG_EN_OVERFLOW where the oracle's cap refused
        assert eng.flags().tolist() == want_flags
        if twin is not None:
            sa, sb = eng.export_state(), twin.export_state()
            for key in sa:
                assert np.array_equal(sa[key], sb[key]), ("state", key)
    finally:
        eng.close()
        if twin is not None:
            twin.close()
