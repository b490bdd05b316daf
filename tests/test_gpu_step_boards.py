"""td_step_boards / TDEngine.step_boards / TDVecEnv.step_boards on the device: one env step for
the boards a caller names, every other board left as it is.

Three yardsticks.  The oracle, directly: one oracle env per board, stepped only in the calls that
name its board (test 1, test 6).  The bystanders: after every call each unnamed board's row of
every output tensor, its exported state, both of its streams and its flags are the bytes they
were, in output buffers that started as a sentinel (test 2, in the runs of test 1).  And a twin
engine stepped in full by td_step, which the rest of the suite pins to the oracle: board b's
j-th partial step equals, bit for bit, board b's j-th full step, through auto-resets (test 3).
B = 37 throughout: no multiple of 8, so the XCD map's remainder branch runs at most list lengths.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import maskutil as M
import skiputil as S
import steputil
from oracle import policies
from oracle import td_oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import envs as E  # noqa: E402
from gym_TD import params as P  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402
from gym_TD.masks import reference_masks  # noqa: E402

lib = _lib.lib
B = 37
OUTPUTS = ("obs", "reward", "done", "win", "allow_next", "cooldowns", "ep_return", "ep_len", "real_def", "fail_def",
           "real_atk", "fail_atk")
FLAG_NO_LAYOUT = 8
SENTINEL = 0x5A


# ------------------------------------------------------------------ helpers
def _cfg(**over):
    cfg = copy.deepcopy(P.config)
    for k, v in over.items():
        setattr(cfg, k, copy.deepcopy(v))
    return cfg


def _engine(L, mode="def", multi=False, seed0=900, cfg=None, autoreset=False, n=B, **kw):
    seeds = list(range(seed0, seed0 + n))
    eng = TDEngine(L, n, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=autoreset, cfg=cfg, **kw)
    eng.reset_all()
    return eng


def _draw(rng, eng):
    """Uniform random actions for every board (multi-action: sparse flags)."""
    L, n = eng.L, eng.B
    d = a = None
    if eng.mode != "atk":
        d = ((rng.random_sample((n, 6, L, L)) < 0.02).astype(np.int64) if eng.multi
             else rng.randint(0, 6 * L * L + 1, size=n).astype(np.int64))
    if eng.mode != "def":
        a = rng.randint(0, 5, size=(n, 3, 8)).astype(np.int64)
    return d, a


def _t(x):
    return None if x is None else torch.from_numpy(x)


def _step(eng, acts):
    eng.step(def_act=_t(acts[0]), atk_act=_t(acts[1]))


def _step_boards(eng, ids, acts):
    return eng.step_boards(ids, def_act=_t(acts[0]), atk_act=_t(acts[1]))


def _subsets(rng, calls, n_boards=B):
    """Board lists for `calls` partial steps: the fixed shapes first -- one board, every board
    (shuffled), 5 and 13 (no multiples of 8) unsorted, runs of adjacent ids, ids whose
    neighbours stay unnamed, the first and the last board -- then random ones, unsorted."""
    fixed = [[17], list(rng.permutation(n_boards)), list(rng.permutation(n_boards)[:5]),
             list(rng.permutation(n_boards)[:13]), [8, 9, 10], [30, 20, 21, 22, 4], [2, 12, 24, 34],
             [0, n_boards - 1], [n_boards - 1, n_boards - 2, 1, 0], sorted(rng.permutation(n_boards)[:13])]
    out = [np.asarray(x, dtype=np.int32) for x in fixed]
    while len(out) < calls:
        k = int(rng.randint(1, n_boards + 1))
        out.append(rng.permutation(n_boards)[:k].astype(np.int32))
    return out[:calls]


def _fill_sentinel(eng):
    """Every output tensor to a byte no step writes a whole row of (needs retain_obs=False)."""
    for name in OUTPUTS:
        t = getattr(eng, name)
        if t is not None:
            t.view(torch.uint8).fill_(SENTINEL)


def _out_bytes(eng):
    """Every output tensor on the host, as [boards, bytes per row]."""
    torch.cuda.synchronize()
    return {n: getattr(eng, n).view(torch.uint8).reshape(eng.B, -1).cpu().numpy()
            for n in OUTPUTS if getattr(eng, n) is not None}


def _outputs(eng, stepped):
    """steputil.outputs for an engine whose unstepped rows still hold the sentinel: its check
    of the AllowNextMove bits on the rows of the boards stepped so far."""
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    out = {n: host(getattr(eng, n)) for n in OUTPUTS}
    out["state"] = eng.export_state()
    assert ((out["allow_next"][np.asarray(stepped)] & 0xFC) == 0).all()
    return out


def _streams(eng, boards):
    return {int(b): (eng.get_py_state(int(b)), eng.get_np_state(int(b))) for b in boards}


class Watch(object):
    """Everything the engine holds, before a call; after it, what may not have moved."""

    def __init__(self, eng, streams=True):
        self.eng, self.with_streams = eng, streams
        self.take()

    def take(self):
        e = self.eng
        self.out = _out_bytes(e)
        self.state = {k: v.copy() for k, v in e.export_state().items()}
        self.flags = e.flags()
        self.streams = _streams(e, range(e.B)) if self.with_streams else None

    def assert_kept(self, boards, tag):
        """Boards `boards` are byte for byte what take() saw; then take() again."""
        old = (self.out, self.state, self.flags, self.streams)
        self.take()
        idx = np.asarray(sorted(boards), dtype=np.int64)
        if len(idx) == 0:
            return
        for name, a in old[0].items():
            assert a[idx].tobytes() == self.out[name][idx].tobytes(), (tag, "output", name)
        for name, a in old[1].items():
            assert a[idx].tobytes() == self.state[name][idx].tobytes(), (tag, "state", name)
        assert (old[2][idx] == self.flags[idx]).all(), (tag, "flags")
        if self.with_streams:
            for b in idx:
                for k in (0, 1):
                    assert np.array_equal(old[3][int(b)][k], self.streams[int(b)][k]), (tag, "stream", int(b), k)


def _others(ids, n_boards=B):
    named = set(int(b) for b in ids)
    return [b for b in range(n_boards) if b not in named]


def _all_bytes_equal(a, b, tag):
    oa, ob = _out_bytes(a), _out_bytes(b)
    for name in oa:
        assert oa[name].tobytes() == ob[name].tobytes(), (tag, "output", name)
    sa, sb = a.export_state(), b.export_state()
    for name in sa:
        assert sa[name].tobytes() == sb[name].tobytes(), (tag, "state", name)
    assert (a.flags() == b.flags()).all(), (tag, "flags")


# ------------------------------------------------------------------ 1 + 2 the oracle, and the bystanders
ORACLE_CASES = [
    (10, "def", False, torch.float32), (10, "atk", False, torch.float32), (10, "2p", False, torch.float32),
    (20, "2p", True, torch.float32), (12, "def", False, torch.float32), (30, "def", False, torch.float32),
    (10, "def", False, torch.float16), (20, "2p", True, torch.float16),
]


@pytest.mark.parametrize("L,mode,multi,dtype", ORACLE_CASES)
def test_subsets_vs_oracle_and_bystanders(L, mode, multi, dtype):
    """40 calls with the lists of _subsets.  Oracle env b steps only in the calls that name board
    b, and after every call every named board equals its oracle env (steputil.check_board:
    reward bits, done, state digest, observation bytes -- the oracle's, rounded to nearest-even
    for float16 --, win, cool-downs, AllowNextMove, RealAction / FailCode), while every unnamed
    board's output rows (sentinel bytes until its first step), exported state, streams and
    flags are byte for byte what they were before the call."""
    seeds, orc = M.ok_seeds(L, B, 3100 + L, S.MODES[mode], multi)
    eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, obs_dtype=dtype,
                   retain_obs=False)
    try:
        _, failed = eng.reset()
        assert not failed
        _fill_sentinel(eng)
        rng = np.random.RandomState(L * 7 + len(mode))
        watch = Watch(eng)
        stepped_once = np.zeros(B, dtype=bool)
        for k, ids in enumerate(_subsets(rng, 40)):
            da, aa = _draw(rng, eng)  # (the unnamed rows hold actions too: they must not be read)
            for b in ids:
                if mode != "atk":
                    da[b] = policies.multi_def(rng, L) if multi else policies.discrete_def(rng, L, orc[b]._board.map[0], 0.5)
                if mode != "def":
                    aa[b] = policies.atk(rng)
            assert _step_boards(eng, ids, (da, aa))[0] is eng.obs
            watch.assert_kept(_others(ids), (L, mode, multi, k))
            stepped_once[ids] = True
            out = _outputs(eng, np.flatnonzero(stepped_once))
            for b in ids:
                o = orc[b]
                if o._board.done():
                    continue  # finished in an earlier call (no auto-reset here)
                d_b = None if da is None else (da[b] if multi else int(da[b]))
                stepped = o.step(d_b, None if aa is None else aa[b])
                want = stepped[0].astype(np.float16) if dtype == torch.float16 else None
                steputil.check_board(eng, out, b, o, stepped, mode, multi, (L, mode, multi, k, int(b)), want_obs=want)
            never = np.flatnonzero(~stepped_once)
            for name, a in watch.out.items():  # rows no call has named yet: still the sentinel
                assert (a[never] == SENTINEL).all(), (k, name)
        assert stepped_once.all()
        assert (eng.flags() == 0).all()
    finally:
        eng.close()


# ------------------------------------------------------------------ 3 the twin, with auto-reset
@pytest.mark.parametrize("L,mode", [(10, "def"), (10, "atk"), (30, "def")])
def test_partial_steps_equal_the_twins_full_steps(L, mode):
    """Engine A steps by subsets, its twin T (same seeds) in full with td_step.  Board b's j-th
    partial step takes the action T's j-th full step gives board b and must leave, bit for bit,
    the outputs T's j-th step left in row b.  Episodes are at most 15 steps, so every board
    auto-resets several times at its own pace.  After 120 calls: the episode records and the
    episode count of A are those of T restricted to the steps each board took; then the
    boards behind are stepped up to the step count of the one in front, after which A and T
    hold the same bytes in every board (state, flags, the opponent stream as CPython's getstate()), and 40 full steps of
    both, through further auto-resets, show that the staged layouts and the layout streams
    behind them are in step too.  (The layout stream's raw position is no yardstick with
    random_agent=True: the refills draw ahead of play, at the launches' cadence.)"""
    hp = M.hyper(False, max_episode_steps=15)
    mk = lambda: _engine(L, mode, seed0=5100, cfg=_cfg(base_LP=2), hp=hp, autoreset=True, retain_obs=False)  # noqa: E731
    a, t = mk(), mk()
    try:
        rng = np.random.RandomState(77 + L)
        calls = _subsets(rng, 120)
        count = np.zeros(B, dtype=np.int64)
        for ids in calls:
            count[ids] += 1
        J = int(count.max())
        acts = [_draw(rng, t) for _ in range(J + 40)]
        names = [n for n in OUTPUTS if getattr(t, n) is not None]
        snaps = {n: torch.empty((J,) + tuple(getattr(t, n).shape), dtype=getattr(t, n).dtype, device=t.device) for n in names}
        states, pys = [], []  # (the opponent stream in CPython's form: the raw words depend on the kernel's lazy twists)
        for j in range(J):
            _step(t, acts[j])
            for n in names:
                snaps[n][j].copy_(getattr(t, n))
            states.append({k: v.copy() for k, v in t.export_state().items() if k != "opp_mt"})
            pys.append(np.stack([t.get_py_state(b) for b in range(B)]))
        host = {n: snaps[n].cpu().numpy() for n in ("done", "ep_return", "ep_len", "win")}
        t_recs = [x.cpu().numpy() for x in t.episode_records()]

        def acts_for(ids, at):
            """Full-batch actions whose rows ids hold the actions of the boards' own next step."""
            d, x = _draw(rng, a)
            for b in ids:
                if d is not None:
                    d[b] = acts[at[b]][0][b]
                if x is not None:
                    x[b] = acts[at[b]][1][b]
            return d, x

        def check_rows(ids, at, tag):
            rows = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=a.device)
            steps = torch.as_tensor(at[ids], device=a.device)
            for n in names:
                got, want = getattr(a, n)[rows].contiguous(), snaps[n][steps, rows].contiguous()
                assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), (tag, n, list(ids), at[ids].tolist())

        done_n = np.zeros(B, dtype=np.int64)
        at = np.zeros(B, dtype=np.int64)
        for k, ids in enumerate(calls):
            _step_boards(a, ids, acts_for(ids, at))
            check_rows(ids, at, k)
            at[ids] += 1
        assert (at == count).all()
        # the episodes A finished: T's, restricted to the steps each board took
        want = [np.zeros(B), np.zeros(B, np.int32), np.full(B, -1, np.int32)]
        for b in range(B):
            for j in range(int(at[b])):
                if host["done"][j][b]:
                    done_n[b] += 1
                    want[0][b], want[1][b], want[2][b] = host["ep_return"][j][b], host["ep_len"][j][b], host["win"][j][b]
        assert (done_n >= 2).all(), done_n.tolist()  # every board auto-reset several times
        got = [x.cpu().numpy() for x in a.episode_records()]
        for w, g in zip(want, got):
            assert w.tobytes() == g.astype(w.dtype).tobytes()
        assert float(a.episode_stats()[0]) == float(done_n.sum())
        # board b after its at[b]-th step is T's board b after T's at[b]-th step
        st = a.export_state()
        for b in range(B):
            for name in states[0]:
                assert st[name][b].tobytes() == states[int(at[b]) - 1][name][b].tobytes(), (b, name)
            assert np.array_equal(a.get_py_state(b), pys[int(at[b]) - 1][b]), (b, "opponent stream")
        # the boards behind catch up; then the two engines are the same bytes, and stay so
        while (at < J).any():
            ids = np.flatnonzero(at < J).astype(np.int32)[::-1].copy()
            _step_boards(a, ids, acts_for(ids, at))
            check_rows(ids, at, "catch-up")
            at[ids] += 1
        sa, sb = a.export_state(), t.export_state()
        for name in states[0]:
            assert sa[name].tobytes() == sb[name].tobytes(), name
        for b in range(B):
            assert np.array_equal(a.get_py_state(b), t.get_py_state(b)), b
        for g, w in zip(a.episode_records(), t_recs):
            assert g.cpu().numpy().tobytes() == w.tobytes()
        sa_, st_ = a.episode_stats().cpu().numpy(), t.episode_stats().cpu().numpy()
        assert sa_[0] == st_[0] and abs(sa_[1] - st_[1]) <= 1e-9 * max(1.0, abs(st_[1]))  # (atomic sum: order free)
        ends = 0
        for j in range(J, J + 40):
            _step(a, acts[j])
            _step(t, acts[j])
            for n in names:
                assert torch.equal(getattr(a, n).view(torch.uint8), getattr(t, n).view(torch.uint8)), (j, n)
            ends += int(t.done.sum().item())
        assert ends >= B  # a further episode end per board, on average: the staged layouts agree
        assert (a.flags() == 0).all() and (t.flags() == 0).all()
    finally:
        a.close()
        t.close()


# ------------------------------------------------------------------ 4 order independence
def test_order_of_the_list_does_not_matter():
    engs = [_engine(10, "2p", retain_obs=False) for _ in range(2)]
    try:
        rng = np.random.RandomState(4)
        for e in engs:
            _fill_sentinel(e)
        for k, ids in enumerate(_subsets(rng, 12)):
            acts = _draw(rng, engs[0])
            _step_boards(engs[0], ids, acts)
            other = ids[::-1].copy() if k % 2 else np.sort(ids)
            if len(ids) > 2 and np.array_equal(other, ids):
                other = np.roll(ids, 1)
            _step_boards(engs[1], other, acts)
            _all_bytes_equal(engs[0], engs[1], k)
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------------ 5 the retained buffer
def _raw(eng, ids, acts, obs=None, n=None, edit=None):
    """td_step_boards itself, on a copy of the engine's io: obs another buffer, n and the ids
    as given (None: NULL), edit(io) last."""
    keep = []
    io = _lib.TdStepIO()
    ctypes.memmove(ctypes.byref(io), ctypes.byref(eng._io), ctypes.sizeof(io))
    if eng.mode != "atk":
        keep.append(torch.from_numpy(acts[0]).to(eng.device))
        io.def_act = keep[-1].data_ptr()
    if eng.mode != "def":
        keep.append(torch.from_numpy(acts[1]).to(eng.device))
        io.atk_act = keep[-1].data_ptr()
    if obs is not None:
        io.obs = obs.data_ptr()
    if edit:
        edit(io)
    arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    rc = lib.td_step_boards(eng._h, io, None if arr is None else arr.ctypes.data, len(arr) if n is None else n,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()  # (the action tensors die with this frame)
    return rc


def test_retained_buffer_equals_the_twins():
    """A retaining engine and its non-retaining twin (every byte written, every step) do the
    same calls; the observation buffers are equal byte for byte after each of them: partial
    steps (boards known, boards not yet known after the buffer was left behind), a copy into
    the retained buffer and a partial step of the copies, a partial step into another buffer
    and then a full step into the retained one, full and partial steps interleaved."""
    engs = [_engine(10, "def", retain_obs=r, autoreset=True, cfg=_cfg(**S.RECIPE)) for r in (True, False)]
    try:
        if not engs[0].retain_obs:
            pytest.skip("TD_RETAIN_OBS=0: no engine retains")
        ret = engs[0].obs.data_ptr()
        assert lib.td_retained_obs(engs[0]._h) == ret and not lib.td_retained_obs(engs[1]._h)
        rng = np.random.RandomState(15)
        lists = _subsets(rng, 30)
        other = [torch.zeros_like(e.obs) for e in engs]

        def same(tag):
            assert lib.td_retained_obs(engs[0]._h) == ret
            assert torch.equal(engs[0].obs.view(torch.uint8), engs[1].obs.view(torch.uint8)), tag

        same("reset")
        for k, ids in enumerate(lists):
            acts = _draw(rng, engs[0])
            if k % 5 == 3:  # a full step between the partial ones
                for e in engs:
                    _step(e, acts)
                same((k, "full"))
            if k == 12:  # fork board 5 into six boards, step the copies only
                kids = [6, 7, 20, 21, 30, 36]
                for e in engs:
                    e.copy_boards([5] * len(kids), kids)
                same((k, "copy"))
                for e in engs:
                    _step_boards(e, kids, acts)
                same((k, "copies stepped"))
            if k == 18:  # into another buffer: the retained one is left behind, rows ids differ now
                for e, buf in zip(engs, other):
                    assert _raw(e, ids, acts, obs=buf) == 0
                assert torch.equal(other[0].view(torch.uint8), other[1].view(torch.uint8))
                acts = _draw(rng, engs[0])
                for e in engs:
                    _step(e, acts)
                same((k, "full after another buffer"))
                continue
            if k == 24:  # left behind again, then partial steps: nothing is known, rows written whole
                for e, buf in zip(engs, other):
                    assert _raw(e, [1, 2], acts, obs=buf) == 0
                acts = _draw(rng, engs[0])
            for e in engs:
                _step_boards(e, ids, acts)
            same(k)  # (rows left stale by a step into another buffer are stale in both)
        for e in engs:
            _step(e, _draw(np.random.RandomState(3), e))
        same("end")
        _all_bytes_equal(engs[0], engs[1], "end")
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------------ 6 after a fork
def test_fork_then_step_the_children():
    """One root fanned out to 12 children, each child given another action, the children
    stepped alone: each equals the oracle's deepcopy of the root stepped with that action; the
    root and the bystanders keep their bytes; the masks of the children are the reference's."""
    L = 10
    cfg = M.config(defender_init_cost=60, defender_cost_rate=2.0, tower_distance=1)  # money for a dozen legal moves
    hp = M.hyper(False)
    seeds, orc = M.ok_seeds(L, B, 7300, O.MODE_DEF, False, cfg=cfg, hp=hp)
    eng = TDEngine(L, B, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, cfg=cfg, hp=hp)
    try:
        assert not eng.reset()[1]
        rng = np.random.RandomState(23)
        root = 16
        for _ in range(25):
            d = np.array([policies.discrete_def(rng, L, o._board.map[0], 0.7) for o in orc], dtype=np.int64)
            _step(eng, (d, None))
            orc[root].step(int(d[root]), None)
        assert not orc[root]._board.done()
        kids = [17, 18, 19, 3, 0, 36, 25, 9, 11, 30, 31, 24]  # next to the root, both ends, runs and loners
        eng.copy_boards([root] * len(kids), kids)
        watch = Watch(eng)
        m = {k: v.cpu().numpy() for k, v in eng.action_mask().items()}
        legal = np.flatnonzero(m["def"][root][:6 * L * L])
        assert len(legal) >= len(kids)
        d = rng.randint(0, 6 * L * L + 1, size=B).astype(np.int64)
        d[kids] = legal[rng.permutation(len(legal))[:len(kids)]]  # a different legal action per child
        d[kids[-1]] = 6 * L * L  # ... and the no-op
        _step_boards(eng, kids, (d, None))
        watch.assert_kept(_others(kids), "fork")
        out = steputil.outputs(eng)
        masks = {k: v.cpu().numpy() for k, v in eng.action_mask(code=True).items()}
        digests = set()
        for b in kids:
            child = copy.deepcopy(orc[root])
            stepped = child.step(int(d[b]), None)
            steputil.check_board(eng, out, b, child, stepped, "def", False, ("child", b))
            dm, dc, _ = reference_masks(M.oracle_state(child), L, cfg, hp, "def", False)
            assert np.array_equal(masks["def"][b], dm) and np.array_equal(masks["def_code"][b], dc), b
            digests.add(out["obs"][b].tobytes())
        assert len(digests) >= len(kids) - 1  # the children went different ways
    finally:
        eng.close()


# ------------------------------------------------------------------ 7 refusals
def test_refusals_change_nothing():
    engs = [_engine(10, "2p", retain_obs=r) for r in (True, False)]
    skip = _engine(10, "def", n=8, frame_skip=2)
    npa = _engine(10, "def", n=8, random_agent=False, autoreset=True)
    try:
        rng = np.random.RandomState(41)
        for _ in range(8):
            acts = _draw(rng, engs[0])
            for e in engs:
                _step(e, acts)
        e = engs[0]
        watch = Watch(e)
        kept = lib.td_retained_obs(e._h)
        acts = _draw(rng, e)

        def null(field):
            return lambda io: setattr(io, field, None)

        bad = [("NULL boards", dict(ids=None, n=1)), ("n < 0", dict(ids=[0], n=-1)),
               ("n > B", dict(ids=list(range(B)) + [0], n=B + 1)), ("id < 0", dict(ids=[3, -1])),
               ("id = B", dict(ids=[B])), ("id = B, last", dict(ids=[0, 1, B])), ("twice", dict(ids=[5, 6, 5])),
               ("twice, ends", dict(ids=[7] + list(range(8, 20)) + [7])),
               ("size", dict(ids=[0], edit=lambda io: setattr(io, "size", io.size - 8))),
               ("abi", dict(ids=[0], edit=lambda io: setattr(io, "abi", 2))),
               ("no obs", dict(ids=[0], edit=null("obs"))), ("no reward", dict(ids=[0], edit=null("reward"))),
               ("no done", dict(ids=[0], edit=null("done"))), ("no def_act", dict(ids=[0], edit=null("def_act"))),
               ("no atk_act", dict(ids=[0], edit=null("atk_act")))]
        for what, kw in bad:
            assert _raw(e, kw.pop("ids"), acts, **kw) < 0, what
            assert lib.td_last_error().startswith(b"td_step_boards"), (what, lib.td_last_error())
        stream = torch.cuda.current_stream().cuda_stream
        ids = (ctypes.c_int32 * 1)(0)
        assert lib.td_step_boards(None, e._io, ids, 1, stream) < 0 and lib.td_step_boards(e._h, None, ids, 1, stream) < 0
        with pytest.raises(_lib.TDError):
            _step_boards(e, [1, 1], acts)
        with pytest.raises(_lib.TDError):
            _step_boards(e, [B], acts)
        for x, word in ((skip, b"frame skip"), (npa, b"random_agent")):
            before = Watch(x, streams=False)
            with pytest.raises(_lib.TDError):
                _step_boards(x, [0, 1], _draw(rng, x))
            assert word in lib.td_last_error(), lib.td_last_error()
            before.assert_kept(range(x.B), word)
        # n == 0 is a no-op: nothing launched, no timing pair taken, nothing written
        e.kernel_timing(2)
        assert _raw(e, [], acts) == 0 and _raw(e, None, acts, n=0) == 0
        assert _step_boards(e, [], acts)[0] is e.obs
        assert len(e.kernel_times()) == 0
        watch.assert_kept(range(B), "refusals")
        assert lib.td_retained_obs(e._h) == kept
        # ... and the next legal calls work, the retained buffer still what the engine thinks it is
        for k, ids in enumerate(_subsets(rng, 4)):
            acts = _draw(rng, e)
            for x in engs:
                _step_boards(x, ids, acts)
            assert torch.equal(engs[0].obs.view(torch.uint8), engs[1].obs.view(torch.uint8)), k
        assert len(e.kernel_times()) == 2  # the two pairs went to the first two kernels
        _all_bytes_equal(engs[0], engs[1], "after refusals")
    finally:
        for x in engs + [skip, npa]:
            x.close()


def test_named_board_without_an_episode():
    """A named board that was never reset behaves as in td_step: zero row, done, TD_FLAG_NO_LAYOUT."""
    import goldens as G
    rows = G.load_roadgen()["10"]
    err = sorted(int(s) for s in rows if "err" in rows[s])[0]
    good = sorted(int(s) for s in rows if "err" not in rows[s])[:7]
    seeds = [err] + good
    eng = TDEngine(10, 8, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, retain_obs=False)
    try:
        assert eng.reset()[1] == [0]
        _fill_sentinel(eng)
        watch = Watch(eng)
        _step_boards(eng, [1, 0], _draw(np.random.RandomState(2), eng))
        watch.assert_kept([2, 3, 4, 5, 6, 7], "no episode")
        assert bool(eng.done[0]) and not bool(eng.obs[0].view(torch.uint8).any()) and float(eng.reward[0]) == 0.0
        assert not bool(eng.done[1]) and bool(eng.obs[1].any())
        fl = eng.flags()
        assert fl[0] == FLAG_NO_LAYOUT and (fl[1:] == 0).all()
    finally:
        eng.close()


def test_unaligned_observation_buffer():
    """An observation buffer off the format's store unit takes the per-element writers: the same
    bytes, and none outside the named rows."""
    engs = [_engine(10, "def", retain_obs=False) for _ in range(2)]
    try:
        rng = np.random.RandomState(12)
        nel = engs[0].obs.numel()
        flat = torch.full((nel + 8,), float("nan"), dtype=torch.float32, device=engs[0].device)
        flat.view(torch.uint8).fill_(SENTINEL)
        off = flat[1:1 + nel].view(engs[0].obs.shape)  # 4 bytes past a 16-B boundary
        assert off.data_ptr() % 16 == 4
        _fill_sentinel(engs[0])
        for k, ids in enumerate(_subsets(rng, 6)[2:]):
            acts = _draw(rng, engs[0])
            _step_boards(engs[0], ids, acts)
            assert _raw(engs[1], ids, acts, obs=off) == 0
            assert torch.equal(off.view(torch.uint8), engs[0].obs.view(torch.uint8)), k
            edge = flat.view(torch.uint8)
            assert bool((edge[:4] == SENTINEL).all()) and bool((edge[4 + 4 * nel:] == SENTINEL).all())
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------------ 8 no host synchronisation needed
def test_back_to_back_equals_synchronised():
    """Five calls with different lists issued back to back on one stream -- more than the handle
    has index slots, the caller's array overwritten right after each call -- against the same
    calls with a device synchronise after each."""
    rng = np.random.RandomState(51)
    lists = [[3, 4, 5], list(range(B))[::-1], [36, 0, 18], [7, 8, 30, 31, 32, 1], [5, 4, 3, 20]]
    engs = [_engine(10, "2p", retain_obs=False) for _ in range(2)]
    try:
        acts = [_draw(rng, engs[0]) for _ in lists]
        dev = [tuple(None if x is None else torch.from_numpy(x).to(engs[0].device) for x in a) for a in acts]
        for sync, e in zip((False, True), engs):
            _fill_sentinel(e)
            torch.cuda.synchronize()
            buf = np.zeros(B, dtype=np.int32)
            for i, ids in enumerate(lists):
                e._io.def_act, e._io.atk_act = dev[i][0].data_ptr(), dev[i][1].data_ptr()
                buf[:len(ids)] = ids
                _lib.check(lib.td_step_boards(e._h, e._io, buf.ctypes.data, len(ids), torch.cuda.current_stream().cuda_stream))
                buf[:] = 0  # the array is the caller's again
                if sync:
                    torch.cuda.synchronize()
        torch.cuda.synchronize()
        _all_bytes_equal(engs[0], engs[1], "back to back")
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------------ 9 the kernel's name, and the upper layers
@pytest.mark.parametrize("L,mode,multi,dtype,want", [
    (10, "def", False, torch.float32, "td_step_sel_kernel<10, 0, false>"),
    (20, "2p", True, torch.float32, "td_step_sel_kernel<20, 2, true>"),
    (12, "atk", False, torch.float32, "td_step_sel_kernel<0, 1, false>"),
    (10, "def", False, torch.float16, "td_step_sel_kernel_f16<10, 0, false>"),
    (30, "def", True, torch.float16, "td_step_sel_kernel_f16<30, 0, true>"),
])
def test_kernel_name(L, mode, multi, dtype, want):
    eng = TDEngine(L, 4, mode, multi, 1, obs_dtype=dtype)
    try:
        assert lib.td_step_boards_kernel_name(eng._h).decode() == want
        eng.set_step_kernel("large")  # (td_step's kernel kind is not td_step_boards')
        assert lib.td_step_boards_kernel_name(eng._h).decode() == want
    finally:
        eng.close()


def test_vector_env_step_boards_and_masks():
    env = E.TDVecEnv(10, 16, "def", seed=300, autoreset=False, action_mask=True)
    twin = E.TDVecEnv(10, 16, "def", seed=300, autoreset=False, action_mask=True)
    try:
        env.reset()
        twin.reset()
        rng = np.random.RandomState(6)
        ids = [9, 2, 3]
        for _ in range(10):
            a = torch.from_numpy(rng.randint(0, 601, size=16).astype(np.int64))
            o, r, dn, info = env.step_boards(ids, a)
            wo, wr, wd, winfo = twin.step(a)
            assert o is env.engine.obs and set(info) == set(winfo)
            for got, want in ((o, wo), (r, wr), (dn, wd), (info["action_mask"], winfo["action_mask"]),
                              (info["RealAction"], winfo["RealAction"])):
                assert torch.equal(got[ids], want[ids])
        rest = [b for b in range(16) if b not in ids]
        assert int(env.engine.export_state()["hdr"]["steps"][rest].max()) == 0
        assert torch.equal(info["action_mask"], env.engine.action_mask()["def"])
    finally:
        env.close()
        twin.close()


def test_host_io_engine():
    """host_io: the call waits for the kernel, the pinned outputs are the caller's on return."""
    seeds = list(range(900, 900 + 8))
    a, t = (TDEngine(10, 8, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, host_io=True)
            for _ in range(2))
    try:
        a.reset_all()
        t.reset_all()
        rng = np.random.RandomState(8)
        for _ in range(10):
            d = rng.randint(0, 601, size=8).astype(np.int64)
            a.step_boards([6, 1], def_act=d)
            t.step(def_act=d)
            for n in ("obs", "reward", "done", "real_def"):
                assert np.array_equal(getattr(a.np, n)[[6, 1]], getattr(t.np, n)[[6, 1]]), n
        assert a.export_state()["hdr"]["steps"].tolist() == [0, 10, 0, 0, 0, 0, 10, 0]
    finally:
        a.close()
        t.close()
