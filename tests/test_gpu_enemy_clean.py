"""The enemy planes of a retained observation are rewritten only when the step touched an
enemy (td_step_obs.h obs_dirty, U::en_touch): a summon, a sort that moved an enemy, a shot that
landed, an enemy entering a new cell.  On every other step their windows are skipped -- and
the buffer must still hold, byte for byte, what a full write leaves.

As tests/test_gpu_obs_retain.py: a retained engine beside a twin built with retain_obs=False,
same seeds and actions, every output compared as bytes after every step.  The main run (10x10,
256 boards, 300 steps, tests/enemyclean.py) is first stepped on the CPU restatement, which
says for every board-step which of the four events happened; the run is refused unless each
kind occurs alone on at least 20 kept board-steps (the sort alone: 3) and 20 are quiet with
an enemy on the board, one of them with a slow-down counter running down (margins change in
all of them).  The engines must follow the restatement's trajectory (done flags and enemy
counts, every step).  The marker test shows that the skip happens: a marker in a window of
enemy planes alone survives exactly the quiet steps."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

import enemyclean as E  # noqa: E402
from gym_TD import _lib  # noqa: E402
from gym_TD import params as P  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402

OUTPUTS = ("obs", "reward", "done", "win", "allow_next", "cooldowns", "ep_return", "ep_len", "real_def", "fail_def",
           "real_atk", "fail_atk")
MAIN_B, MAIN_STEPS = 256, 300


@functools.lru_cache(maxsize=1)
def _main():
    """The main run's restatement, once for every test that follows it."""
    tr = E.Trace(10, MAIN_B, "def", False, MAIN_STEPS)
    tr.check()
    return tr


def _hp(multi):
    hp = P.HyperParameters()
    object.__setattr__(hp, "max_episode_steps", E.EP)
    object.__setattr__(hp, "allow_multiple_actions", bool(multi))
    return hp


def _cfg(L):
    c, o = copy.deepcopy(P.config), E.oracle_cfg(L)
    for name in ("enemy_speed", "attacker_init_cost", "defender_init_cost", "defender_cost_rate"):
        setattr(c, name, copy.deepcopy(getattr(o, name)))
    return c


def _engine(L, seeds, mode, multi, kernel, dtype, retain, **kw):
    return TDEngine(L, len(seeds), mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, cfg=_cfg(L),
                    hp=_hp(multi), step_kernel=kernel, obs_dtype=dtype, retain_obs=retain, **kw)


def _pair(L, seeds, mode="def", multi=False, kernel="auto", dtype=torch.float32, **kw):
    a = _engine(L, seeds, mode, multi, kernel, dtype, True, **kw)
    b = _engine(L, seeds, mode, multi, kernel, dtype, False, **kw)
    assert a.retain_obs and _lib.lib.td_retained_obs(a._h) == a.obs.data_ptr()
    assert not b.retain_obs and _lib.lib.td_retained_obs(b._h) is None
    a.reset_all()
    b.reset_all()
    _same(a, b, "reset")
    return a, b


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, where):
    """Every output of engine a equals engine b's, as bytes (every board's row)."""
    for name in OUTPUTS:
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), name
        if ta is None or torch.equal(_bytes(ta), _bytes(tb)):
            continue
        if name == "obs":
            diff = (_bytes(ta) != _bytes(tb)).reshape(a.B, 45, -1).any(dim=2).cpu().numpy()
            bd = np.flatnonzero(diff.any(axis=1))
            raise AssertionError(("observation bytes", where, "boards", bd[:8].tolist(), "channels of the first",
                                  np.flatnonzero(diff[bd[0]]).tolist()))
        raise AssertionError((name, where))


def _dev(eng, x):
    return None if x is None else torch.from_numpy(x).to(eng.device)


def _finish(a, b):
    sa, sb = a.export_state(), b.export_state()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), ("state", key)
    assert (a.flags() == 0).all() and (b.flags() == 0).all()


def _seeds(L, B, mode, multi, seed0):
    """The first B seeds from seed0 whose first layout draw succeeds (no restatement run)."""
    return E.Trace(L, B, mode, multi, steps=0, seed0=seed0).seeds


# ------------------------------------------------------------------ the twin comparisons
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("kernel", ["large", "small", "small2"])
def test_main_run_equals_its_twin(kernel, dtype):
    tr = _main()
    a, b = _pair(10, tr.seeds, kernel=kernel, dtype=dtype)
    try:
        assert a.step_kernel == b.step_kernel == kernel
        for k in range(tr.steps):
            d = _dev(a, tr.def_act[k])
            a.step(d)
            b.step(d)
            _same(a, b, k)
            # the restatement's trajectory: what it calls quiet is quiet here
            assert np.array_equal(b.done.cpu().numpy().astype(bool), tr.done[k]), ("done", k)
            if k % 25 == 24 or k == tr.steps - 1:
                n_en = b.export_state()["hdr"]["n_en"]
                keep = ~tr.done[k]
                assert np.array_equal(n_en[keep], tr.n_en[k][keep]), ("enemy counts", k)
        _finish(a, b)
    finally:
        a.close()
        b.close()


def _random_twin(L, B, mode, multi, steps, seed0, **kw):
    """A twin run on actions drawn here; returns how many board-steps had an enemy."""
    seeds = _seeds(L, B, mode, multi, seed0)
    a, b = _pair(L, seeds, mode, multi, **kw)
    try:
        rng, with_enemy = np.random.RandomState(11), 0
        for k in range(steps):
            d, at = E.draw_actions(rng, L, B, mode, multi)
            d, at = _dev(a, d), _dev(a, at)
            a.step(d, at)
            b.step(d, at)
            _same(a, b, k)
            if k % 10 == 9:
                with_enemy += int((b.export_state()["hdr"]["n_en"] > 0).sum())
        _finish(a, b)
        return with_enemy
    finally:
        a.close()
        b.close()


def test_frame_skip_3():
    """k = 3: one observation for three board steps, the touched bit ORed over them."""
    assert _random_twin(10, 33, "def", False, 100, 7300, frame_skip=3) > 0


def test_2p_20x20_multi_action():
    """The attacker's clusters are the caller's (attacker_actions), the defender scans."""
    assert _random_twin(20, 9, "2p", True, 60, 7300) > 0


def test_def_30x30():
    assert _random_twin(30, 9, "def", False, 60, 7300) > 0


@pytest.mark.parametrize("form", ["host", "dev"])
def test_partial_steps(form):
    """step_boards / step_boards_dev: a random half of the boards per call; the rows of the
    named and of the unnamed boards are all compared."""
    tr = _main()
    B = 64
    a, b = _pair(10, tr.seeds[:B])
    try:
        rng = np.random.RandomState(5)
        for k in range(150):
            d = _dev(a, tr.def_act[k][:B].copy())
            ids = np.flatnonzero(rng.random_sample(B) < 0.5).astype(np.int32)
            rng.shuffle(ids)
            for e in (a, b):
                if form == "host":
                    e.step_boards(ids, d)
                else:
                    e.step_boards_dev(torch.from_numpy(ids).to(e.device), d)
            _same(a, b, k)
        assert a.list_errors() == (0, None) and b.list_errors() == (0, None)
        _finish(a, b)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ the skip happens
# Board unit 700 (channel 28 -- the minimum plane of enemy type 3 -- cells 0-3): at every one of
# a 10x10 board's 8 line misalignments its window (stream units 640-767) holds enemy planes
# alone (units 625-1024 of the board), so only the enemy class can have it written.
MARK_CH, MARK = 28, 7.0


@pytest.mark.parametrize("kernel", ["large", "small", "small2"])
def test_marker_survives_exactly_the_quiet_steps(kernel):
    tr = _main()
    quiet, kept = tr.quiet(), tr.kept()
    k0 = next(k for k in range(50, tr.steps - 45) if quiet[k].sum() >= 8)
    marked = np.flatnonzero(quiet[k0])
    a, b = _pair(10, tr.seeds, kernel=kernel)
    try:
        for k in range(k0):
            d = _dev(a, tr.def_act[k])
            a.step(d)
            b.step(d)
        _same(a, b, k0 - 1)
        idx = torch.from_numpy(marked).to(a.device)
        for e in (a, b):
            e.obs[idx, MARK_CH, 0, 0:4] = MARK
        alive = np.ones(len(marked), dtype=bool)  # every step since the marker was quiet
        survived = overwritten = 0
        for k in range(k0, k0 + 45):
            d = _dev(a, tr.def_act[k])
            a.step(d)
            b.step(d)
            was = alive.copy()
            alive &= quiet[k, marked]
            oa, ob = a.obs.cpu().numpy(), b.obs.cpu().numpy()
            assert (ob[marked, MARK_CH, 0, 0:4] != MARK).all(), ("the twin kept a marker", k)
            got = (oa[marked, MARK_CH, 0, 0:4] == MARK).all(axis=1)
            assert np.array_equal(got, alive), ("marker", k, marked[got != alive].tolist())
            survived += int(alive.sum())
            # a step that touched an enemy of a board that kept its episode ended the marker
            overwritten += int((was & ~alive & kept[k, marked]).sum())
            oa[marked[alive], MARK_CH, 0, 0:4] = ob[marked[alive], MARK_CH, 0, 0:4]
            assert np.array_equal(oa.view(np.uint32), ob.view(np.uint32)), ("everything else as the twin", k)
            if not alive.any():
                break
        assert survived >= len(marked) and overwritten >= 1, (survived, overwritten)
        assert not alive.any(), "45 steps are longer than an episode"
    finally:
        a.close()
        b.close()
