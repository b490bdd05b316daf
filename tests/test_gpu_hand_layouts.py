"""Hand-made layouts on the device: the catalogue of tests/handmaps.py, handed over with
td_layout_from_roads + td_reset_layouts and stepped against HandEnv, bit for bit -- on every
step kernel the size has, and (`snake64`, whose far cells read the last entry of the kernels'
distance table, and `cross`, where a road overwrites another's distances) through frame skip,
the float16 observation, the retained observation and a 4-B-aligned buffer.  Then what the
boundary refuses on a live handle, and TD_FLAG_BAD_MOVE.

Auto-reset is off: the test restarts finished boards itself with reset_layouts, together with
HandEnv.reset().  tests/test_hand_layout_ref.py shows on the oracle alone that each run
reaches what its map was drawn for."""
import numpy as np
import pytest
import torch

import handmaps as H
import skiputil as S
import steputil
from oracle import canon

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402

from test_gpu_frame_skip import _compare as compare_macro  # noqa: E402

FLAG_BAD_MOVE = 16


def _engine(L, mode, difficulty, over, recs, kernel="auto", **kw):
    """An engine of len(recs) boards, board b restarted from recs[b]; its opponent streams are
    the HandEnvs' (H.OPP_SEED0 + b)."""
    B = len(recs)
    eng = TDEngine(L, B, mode, False, difficulty, np_seeds=np.arange(B) + 1, py_seeds=np.arange(B) + H.OPP_SEED0,
                   autoreset=False, cfg=H.config(**over), hp=H.hyper(), step_kernel=kernel, **kw)
    try:
        if kernel != "auto":
            assert eng.step_kernel == kernel
        eng.reset_layouts(np.stack(recs), np.arange(B))
    except Exception:
        eng.close()
        raise
    return eng


def _case_engine(case, kernel="auto", n=None, **kw):
    _, _, mode, difficulty, over, _, steps = H.CASE[case]
    L, roads, envs = H.make_envs(case, n)
    rec = H.record(roads, L)
    return _engine(L, mode, difficulty, over, [rec] * len(envs), kernel, **kw), envs, rec, mode, L, steps


def _step(eng, da, aa):
    eng.step(def_act=None if da is None else torch.from_numpy(da), atk_act=None if aa is None else torch.from_numpy(aa))


def _want(obs, f16):
    return obs.astype(np.float16) if f16 else obs


def _restart(eng, envs, recs, boards, f16=False):
    """reset_layouts + HandEnv.reset() of ``boards``; the fresh observation and state compared."""
    if not len(boards):
        return
    obs = eng.reset_layouts(np.stack([recs[b] for b in boards]), boards).cpu().numpy()
    for b in boards:
        H.note_end(envs[b])
        want = _want(envs[b].reset(), f16)
        assert np.array_equal(obs[b], want), ("restart", b, np.argwhere(obs[b] != want)[:5].tolist())
        assert canon.state_digest(eng.board_state(b)) == canon.state_digest(canon.oracle_state(envs[b])), ("restart", b)


def _play(eng, envs, recs, mode, steps, f16=False, first=0):
    """``steps`` steps of H.draw_actions on the engine and on its HandEnvs, every board compared
    at every step (steputil.check_board), finished boards restarted."""
    L = eng.L
    rng = np.random.RandomState(L)
    for k in range(first, first + steps):
        da, aa = H.draw_actions(rng, mode, envs, L)
        _step(eng, da, aa)
        out = steputil.outputs(eng)
        done = []
        for b, o in enumerate(envs):
            stepped = o.step(None if da is None else int(da[b]), None if aa is None else aa[b])
            steputil.check_board(eng, out, b, o, stepped, mode, False, (mode, k, b), want_obs=_want(stepped[0], f16))
            if stepped[2]:
                done.append(b)
        _restart(eng, envs, recs, done, f16)


_PARITY = [(c[0], k) for c in H.CASES
           for k in (("large", "small", "small2") if H.MAPS[c[1]][0] in (10, 20) else ("large",))]


@pytest.mark.parametrize("case,kernel", _PARITY)
def test_catalogue_vs_oracle(case, kernel):
    """Every board of a catalogue case against its HandEnv at every step: reward bits, done,
    state digest, every observation byte, win, cool-downs, AllowNextMove, RealAction /
    FailCode; flags 0 at the end.  On the parent's library `cross` fails at its first
    observation: the record's max dist was 17 (the maximum over all writes) where the finished
    plane's is 16, so channel 9 was divided by 18."""
    eng, envs, rec, mode, L, steps = _case_engine(case, kernel)
    try:
        obs = eng.obs.cpu().numpy()
        for b, o in enumerate(envs):
            assert np.array_equal(obs[b], o._board.get_states()), ("first observation", b)
        _play(eng, envs, [rec] * len(envs), mode, steps)
        assert (eng.flags() == 0).all()
        assert H.merged_trace(envs)["episodes"] >= 3
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["snake64", "cross"])
@pytest.mark.parametrize("path", ["f16", "offset4"])
def test_far_cells_on_other_observation_writers(case, path):
    """The same comparison through the float16 writers (expected: the oracle's float32
    observation cast to float16) and into a buffer 4 bytes off 16-B alignment (the per-element
    path); nothing is written outside that buffer."""
    f16 = path == "f16"
    eng, envs, rec, mode, L, steps = _case_engine(case, obs_dtype=torch.float16 if f16 else torch.float32)
    try:
        big = None
        if not f16:
            n = eng.B * _lib.NCH * L * L
            big = torch.full((n + 2,), -1.0, device="cuda")
            eng.set_obs_dtype(torch.float32, big[1:-1].view(eng.B, _lib.NCH, L, L))
            assert eng.obs.data_ptr() % 16 == 4
            eng.reset_layouts(np.stack([rec] * eng.B), np.arange(eng.B))
        else:
            assert "_f16<" in eng.step_kernel_name
        _play(eng, envs, [rec] * len(envs), mode, steps, f16)
        assert (eng.flags() == 0).all()
        if big is not None:
            assert float(big[0]) == -1.0 and float(big[-1]) == -1.0
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["snake64", "cross"])
def test_far_cells_retained_observation(case):
    """retain_obs=True (a step skips the windows it knows unchanged) against a twin engine that
    writes every byte, over the same actions and across reset_layouts of finished boards and,
    every 16th step, of two boards in the middle of an episode."""
    a, envs, rec, mode, L, steps = _case_engine(case, retain_obs=True)
    b = None
    try:
        b = _case_engine(case, retain_obs=False)[0]
        assert a.retain_obs and not b.retain_obs
        assert torch.equal(a.obs, b.obs)
        rng = np.random.RandomState(L)
        restarts = 0
        for k in range(steps):
            da, aa = H.draw_actions(rng, mode, envs, L)
            _step(a, da, aa)
            _step(b, da, aa)
            assert torch.equal(a.obs, b.obs), k
            assert torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), k
            for i, o in enumerate(envs):  # (the oracle only feeds draw_actions its road map)
                o.step(None if da is None else int(da[i]), None if aa is None else aa[i])
            done = np.flatnonzero(a.done.cpu().numpy()).tolist()
            if k % 16 == 15:
                done = sorted(set(done) | {1, 2})
            if done:
                for eng in (a, b):
                    eng.reset_layouts(np.stack([rec] * len(done)), done)
                for i in done:
                    envs[i].reset()
                restarts += len(done)
                assert torch.equal(a.obs, b.obs), ("restart", k)
        assert restarts >= 5
        want = np.stack([o._board.get_states() for o in envs])
        assert np.array_equal(a.obs.cpu().numpy(), want)
    finally:
        a.close()
        if b is not None:
            b.close()


class HandRef(S.Ref):
    """skiputil's sub-stepped reference on a HandEnv (the Python oracle alone)."""

    def __init__(self, env, mode):
        self.L, self.mode, self.multi = env.L, mode, False
        self.c, self.o = None, env
        self.ep_ret, self.ep_len = 0.0, 0
        self.empty_def = 6 * env.L * env.L
        self.empty_atk = np.full((3, 8), 4, dtype=np.int64)
        self.autoreset = False


@pytest.mark.parametrize("case", ["snake64", "cross"])
def test_far_cells_frame_skip(case):
    """Frame skip 3: the skip kernels keep raw cell words where the step kernels keep packed
    ones, and swap them around the distance bits.  Against the oracle stepped sub-step by
    sub-step (skiputil.Ref.macro), a finished board restarted by the test."""
    k = 3
    eng, envs, rec, mode, L, steps = _case_engine(case, frame_skip=k)
    try:
        refs = [HandRef(o, mode) for o in envs]
        rng = np.random.RandomState(L)
        ends = 0
        for i in range(steps // k):
            da, aa = H.draw_actions(rng, mode, envs, L)
            _step(eng, da, aa)
            outs = [r.macro(k, None if da is None else int(da[b]), None if aa is None else aa[b])
                    for b, r in enumerate(refs)]
            compare_macro(eng, outs, (case, i))
            st = eng.export_state()
            for b, o in enumerate(envs):
                assert canon.state_digest(eng.board_state(b, st)) == canon.state_digest(canon.oracle_state(o)), (i, b)
            done = [b for b, out in enumerate(outs) if out["done"]]
            _restart(eng, envs, [rec] * len(envs), done)
            for b in done:
                refs[b].ep_ret, refs[b].ep_len = 0.0, 0
            ends += len(done)
        assert ends >= 3
        assert (eng.flags() == 0).all()
    finally:
        eng.close()


# ------------------------------------------------------------------ refusals on a live handle
def _raw(eng):
    st = eng.export_state()
    return {k: np.array(v, copy=True) for k, v in st.items()}


def _same(x, y):
    return all(x[k].tobytes() == y[k].tobytes() for k in x)


def test_boundary_refuses_on_a_live_handle():
    """td_reset_layouts with a record whose max dist is 64 or whose num_roads is 0, and
    td_import_state of an export whose header says max dist 64, return < 0 with a message and
    change nothing: the exported state of every board, the flags and the retained observation
    are what they were -- also for the board whose good record came first in the same call --
    and the next step still matches the oracle.  (On the parent's library all three are taken.)"""
    eng, envs, rec, mode, L, _ = _case_engine("cross", n=8)
    try:
        _play(eng, envs, [rec] * 8, mode, 12)
        before, obs0, flags0 = _raw(eng), eng.obs.clone(), eng.flags().copy()
        far, none = rec.copy(), rec.copy()
        far[3], none[1] = 64, 0
        for bad, msg in ((far, "max dist 64"), (none, "num_roads 0")):
            with pytest.raises(_lib.TDError, match=msg):
                eng.reset_layouts(np.stack([rec, bad]), [0, 3])
            assert _same(_raw(eng), before) and torch.equal(eng.obs, obs0) and (eng.flags() == flags0).all(), msg
        recs = np.ascontiguousarray(np.stack([far]), dtype=np.uint32)
        ids = np.array([2], dtype=np.int32)
        assert _lib.lib.td_reset_layouts(eng._h, _lib.ptr(recs, _lib.ctypes.c_uint32), _lib.ptr(ids, _lib.ctypes.c_int32),
                                         1, eng.obs.data_ptr(), None) < 0
        for value in (64, -1):
            st = _raw(eng)
            st["hdr"][5]["maxdist"] = value
            with pytest.raises(_lib.TDError, match="board 5: max dist"):
                eng.import_state(st)
            assert _same(_raw(eng), before) and torch.equal(eng.obs, obs0) and (eng.flags() == flags0).all(), value
        eng.import_state(before)  # (max dist 16: taken)
        assert _same(_raw(eng), before)
        _play(eng, envs, [rec] * 8, mode, 12, first=12)
        assert (eng.flags() == 0).all()
    finally:
        eng.close()


# ------------------------------------------------------------------ TD_FLAG_BAD_MOVE
def test_bad_move_flag_and_rule():
    """A road that dead-ends on the right edge (odd boards; against the layout rule on purpose):
    the enemy that would leave the board stays on its cell, with the margin already reduced by
    1, the board's flag word gains TD_FLAG_BAD_MOVE in that very step and keeps it until
    reset_layouts of that board clears it.  Odd and even boards are compared bit for bit with
    the oracle, whose Board restates the rule as an opt-in (stay_on_bad_move)."""
    L, roads, envs = H.bad_move_envs()
    recs = [H.try_record(r, L)[1] for r in roads]
    assert all(int(r[0]) == 0x7D1A0001 for r in recs)
    eng = _engine(L, "atk", 1, {}, recs)
    try:
        rng = np.random.RandomState(L)
        gained = cleared = 0
        for k in range(H.BAD_MOVE_STEPS):
            _, aa = H.draw_actions(rng, "atk", envs, L)
            had = [o._board.bad_move for o in envs]
            _step(eng, None, aa)
            out = steputil.outputs(eng)
            done = []
            for b, o in enumerate(envs):
                stepped = o.step(None, aa[b])
                steputil.check_board(eng, out, b, o, stepped, "atk", False, (k, b))
                if stepped[2]:
                    done.append(b)
            flags = eng.flags()
            assert flags.tolist() == [FLAG_BAD_MOVE if o._board.bad_move else 0 for o in envs], k
            gained += sum(o._board.bad_move and not h for o, h in zip(envs, had))
            cleared += sum(envs[b]._board.bad_move for b in done)
            _restart(eng, envs, recs, done)
            assert all(eng.flags()[b] == 0 for b in done), k
        assert gained >= 4 and cleared >= 4, (gained, cleared)
        assert not any(o.trace["episodes"] == 0 for o in envs)
    finally:
        eng.close()
