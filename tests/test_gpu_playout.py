"""Random playouts on the device (td_playout[_boards[_dev]] / TDEngine.playout*) against a twin
engine with the same seeds that runs the loop the playout is defined by: sample_actions_boards at
ticket + j, then step_boards, over the boards not yet done.

Compared over all boards: the reward's bits (the twin adds left to right in f64), done, steps_run,
win, allow_next, cooldowns, ep_return, ep_len; the exported state, both streams of every board,
the flags, the episode statistics and records (streamutil.snapshot); and after that one full
step of both engines with equal actions, whose observation must agree byte for byte -- which
also shows that the playout left the retained buffer behind.  The oracle anchor compares with
gym_TD.sampling.reference_playout on the CPU oracle itself (tests/playoutref.py)."""
import numpy as np
import pytest
import torch

import cfgspace
import maskutil as M
import playoutref as PR
import sampleutil as U
import streamutil as SU

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import envs as E  # noqa: E402
from gym_TD import sampling as S  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402
from test_gpu_action_mask import _engine, _restart_7  # noqa: E402

SEED = 7
OUT = ("reward", "done", "steps_run", "win", "allow_next", "cooldowns", "ep_return", "ep_len")
STEP_OUT = ("done", "win", "allow_next", "cooldowns", "ep_return", "ep_len")


def _pair(L, B, mode, cfg, hp, autoreset, seed0=500):
    a = _engine(L, B, mode, False, cfg, hp, autoreset, seed0)
    b = _engine(L, B, mode, False, cfg, hp, autoreset, seed0)
    a.sample_seed = b.sample_seed = SEED
    return a, b


def _drive(engs, boards, ticket, idle=0.3):
    """One sampled step of ``boards`` on every engine (the same step: same seeds, same ticket)."""
    boards = np.asarray(boards, dtype=np.int32)
    for e in engs:
        out = e.sample_actions_boards(boards, ticket=ticket, def_idle=idle, atk_idle=idle)
        e.step_boards(boards, def_act=out["def"], atk_act=out["atk"])


def _phase_shift(engs, k, limit):
    """Boards phase-shifted by b mod k: board b is stepped to limit - 1 - b mod min(k, limit) steps
    of its episode, so the step limit ends episodes at every sub-step position."""
    m = max(1, min(k, limit))
    pre = limit - 1 - np.arange(engs[0].B) % m
    for p in range(int(pre.max())):
        _drive(engs, np.flatnonzero(pre > p), 5000 + p)


def _twin_loop(tw, boards, k, ticket, di, ai, never=()):
    """The loop a playout is defined by, on the twin; what the playout's outputs must be."""
    B = tw.B
    res = {"reward": np.zeros(B), "done": np.zeros(B, np.uint8), "steps_run": np.zeros(B, np.int32),
           "win": np.zeros(B, np.int8), "allow_next": np.zeros(B, np.uint8), "cooldowns": np.zeros(B, np.uint8),
           "ep_return": np.zeros(B), "ep_len": np.zeros(B, np.int32)}
    alive = np.asarray(boards, dtype=np.int32)
    for j in range(k):
        if not len(alive):
            break
        out = tw.sample_actions_boards(alive, ticket=(ticket + j) & S.M64, def_idle=di, atk_idle=ai)
        tw.step_boards(alive, def_act=out["def"], atk_act=out["atk"])
        r = tw.reward.cpu().numpy()
        res["reward"][alive] = r[alive] if j == 0 else res["reward"][alive] + r[alive]
        for n in STEP_OUT:
            res[n][alive] = getattr(tw, n).cpu().numpy()[alive]
        res["steps_run"][alive] += 1
        alive = alive[res["done"][alive] == 0]
    res["steps_run"][list(never)] = 0  # a board never reset runs no sub-step (the twin's step reports it done)
    return res


def _state(eng):
    return {k: v for k, v in SU.snapshot(eng).items() if not k.startswith("out.")}


def _same_outputs(got, want, rows, where):
    for n in OUT:
        g, w = got[n].cpu().numpy()[rows], want[n][rows]
        if n in ("reward", "ep_return"):
            g, w = g.view(np.uint64), w.view(np.uint64)
        bad = np.flatnonzero(g != w)
        assert not len(bad), (where, n, "board", int(np.asarray(rows)[bad[0]]), g[bad[0]], w[bad[0]], len(bad))


def _full_step_equal(a, b, where, np_lead):
    """One full step of both engines with equal (sampled) actions: every output, the observation
    included, byte for byte."""
    for e in (a, b):
        out = e.sample_actions(ticket=999999, def_idle=0.3, atk_idle=0.3)
        e.step(def_act=out["def"], atk_act=out["atk"])
    SU.same(SU.snapshot(a), SU.snapshot(b), where + " / full step", np_lead=np_lead)


def _check(a, b, k, ticket, di, ai, where, boards=None, never=(), dev=None, first=False, full_step=True):
    """Playout on ``a`` (every board, a host list, or dev = (ids, count) tensors), the loop on
    ``b``; everything compared."""
    np_lead = bool(a.autoreset)
    if dev is not None:
        got = a.playout_boards_dev(dev[0], k, count=dev[1], ticket=ticket, def_idle=di, atk_idle=ai, first=first)
    else:
        got = a.playout(k, boards, ticket=ticket, def_idle=di, atk_idle=ai, first=first)
    rows = np.arange(a.B) if boards is None else np.asarray(boards, dtype=np.int64)
    want = _twin_loop(b, rows, k, ticket, di, ai, never)
    _same_outputs(got, want, rows, where)
    SU.same(_state(a), _state(b), where, np_lead=np_lead)
    if full_step:
        _full_step_equal(a, b, where, np_lead)
    return got, want


# ------------------------------------------------------------------------------ 1: base sweep
_VARIANTS = [(True, 0, 0), (False, U.IDLE_03, 2), (True, U.IDLE_03, 3), (False, 0, 3), (True, U.IDLE_03, 0)]
_IVS = (0, 2, 3)


@pytest.mark.parametrize("mode", ["def", "atk", "2p"])
@pytest.mark.parametrize("q,k", list(enumerate([1, 2, 5, 16, 64])))
def test_base_sweep(mode, q, k):
    """48 boards of 10x10, episodes of 23 steps, boards phase-shifted by b mod k.  Over the five k
    of a mode: auto-reset on and off, idle 0 and IDLE_03, action intervals 0, 2 and 3."""
    autoreset, idle, iv = _VARIANTS[q]
    iv = _IVS[(_IVS.index(iv) + ["def", "atk", "2p"].index(mode)) % 3]
    cfg = M.config(M.RICH, M.ATK, defender_action_interval=iv, attacker_action_interval=iv)
    hp = M.hyper(max_episode_steps=23)
    a, b = _pair(10, 48, mode, cfg, hp, autoreset)
    try:
        _phase_shift((a, b), k, 23)
        got, want = _check(a, b, k, 100, idle, idle, "sweep %s k=%d" % (mode, k))
        print("sweep %s k=%d: steps_run %s, done %d" % (mode, k, np.bincount(want["steps_run"]), int(want["done"].sum())))
        if k >= 5:
            assert len(set(want["steps_run"][want["done"] == 1])) >= min(k, 5)  # ends at several positions
        assert (a.flags() == 0).all()
        # a second playout from the state the first one left (new episodes under auto-reset)
        _check(a, b, k, 300, idle, idle, "sweep %s k=%d again" % (mode, k), full_step=False)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------ 2: other sizes
@pytest.mark.parametrize("L,mode", [(20, "2p"), (30, "def"), (30, "atk"), (12, "atk"), (12, "def"), (7, "2p")])
def test_other_sizes(L, mode):
    """16 boards at 20x20 and 30x30, and at 12x12 and 7x7 (the generic build, NC & 3 zero and not)."""
    cfg = M.config(M.RICH, M.ATK)
    hp = M.hyper(max_episode_steps=23)
    a, b = _pair(L, 16, mode, cfg, hp, L != 7)
    try:
        _phase_shift((a, b), 5, 23)
        for r in range(5):  # several playouts in a row: towers stand, enemies walk, episodes end
            _check(a, b, 5, 100 + 5 * r, 0, U.IDLE_03, "L=%d %s r=%d" % (L, mode, r), full_step=r == 4)
            if L == 7:
                done = np.flatnonzero(a.done.cpu().numpy() | (a._playout_buf["done"].cpu().numpy() != 0))
                for e in (a, b):
                    _restart_7(e, done)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 3: split, reproducible, first
def test_split():
    """k = 40 from ticket t, against 20 and then 20 more at t + 20 for the boards not done: the
    same states, streams and counts (the reward is two partial sums there: equal to rounding)."""
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=50)
    a, b = _pair(10, 48, "2p", cfg, hp, False)
    try:
        _phase_shift((a, b), 48, 40)
        one = {n: v.cpu().numpy().copy() for n, v in a.playout(40, ticket=70, def_idle=0.3).items() if v is not None}
        p1 = {n: v.cpu().numpy().copy() for n, v in b.playout(20, ticket=70, def_idle=0.3).items() if v is not None}
        rest = np.flatnonzero(p1["done"] == 0)
        assert 0 < len(rest) < 48
        p2 = {n: v.cpu().numpy().copy() for n, v in b.playout(20, rest, ticket=90, def_idle=0.3).items() if v is not None}
        SU.same(_state(a), _state(b), "split")
        run = p1["steps_run"].copy()
        run[rest] += p2["steps_run"][rest]
        assert np.array_equal(one["steps_run"], run) and np.array_equal(one["done"], p2["done"])
        rew = p1["reward"].copy()
        rew[rest] += p2["reward"][rest]
        assert np.allclose(one["reward"], rew, rtol=1e-12, atol=1e-9)
        assert np.array_equal(one["ep_return"].view(np.uint64), p2["ep_return"].view(np.uint64))
        assert (one["steps_run"][one["done"] == 0] == 40).all()
    finally:
        a.close()
        b.close()


def test_reproducible_and_first_actions():
    """The same seed and ticket give the same playout; another ticket, from the same pre-state on a
    third engine, other first actions; first_def / first_atk are td_sample_actions' rows at
    `ticket` on the pre-state."""
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=23)
    a, b = _pair(10, 48, "2p", cfg, hp, True)
    c = _engine(10, 48, "2p", False, cfg, hp, True)
    c.sample_seed = SEED
    try:
        _phase_shift((a, b, c), 16, 23)
        want = {n: v.cpu().numpy().copy() for n, v in a.sample_actions(ticket=40, def_idle=0.3, atk_idle=0.3).items()
                if v is not None}
        other = {n: v.cpu().numpy().copy() for n, v in a.sample_actions(ticket=41, def_idle=0.3, atk_idle=0.3).items()
                 if v is not None}
        ga = {n: v.cpu().numpy().copy() for n, v in a.playout(16, ticket=40, def_idle=0.3, atk_idle=0.3, first=True).items()}
        gb = {n: v.cpu().numpy().copy() for n, v in b.playout(16, ticket=40, def_idle=0.3, atk_idle=0.3, first=True).items()}
        gc = {n: v.cpu().numpy().copy() for n, v in c.playout(16, ticket=41, def_idle=0.3, atk_idle=0.3, first=True).items()}
        for n in ga:
            assert np.array_equal(ga[n].view(np.uint8), gb[n].view(np.uint8)), n
        SU.same(_state(a), _state(b), "reproducible", np_lead=True)
        assert np.array_equal(ga["first_def"], want["def"]) and np.array_equal(ga["first_atk"], want["atk"])
        assert (ga["first_def"] != 600).any() and (ga["first_atk"][:, :, 0] != 4).any()
        # the playout at another ticket: the sampler's rows at that ticket, and not the first one's
        assert np.array_equal(gc["first_def"], other["def"]) and np.array_equal(gc["first_atk"], other["atk"])
        assert (gc["first_def"] != ga["first_def"]).any() and (gc["first_atk"] != ga["first_atk"]).any()
        assert (gc["reward"].view(np.uint64) != ga["reward"].view(np.uint64)).any()
    finally:
        a.close()
        b.close()
        c.close()


def test_ticket_none_takes_the_engines_counter():
    """ticket=None starts at the engine's sampling counter and advances it by `steps`, for all
    three calls; a refused call takes no ticket."""
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=23)
    a, b = _pair(10, 32, "2p", cfg, hp, True)
    try:
        a._sample_ticket = b._sample_ticket = t0 = S.M64 - 2  # (across the wrap)
        ids = np.arange(1, 30, 2, dtype=np.int32)
        dev = torch.from_numpy(ids).to(a.device)
        ga = {n: v.cpu().numpy().copy() for n, v in a.playout(5, first=True).items()}
        assert a._sample_ticket == (t0 + 5) & S.M64 == 2
        gb = {n: v.cpu().numpy().copy() for n, v in b.playout(5, ticket=t0, first=True).items()}
        assert b._sample_ticket == t0  # an explicit ticket leaves the counter alone
        for n in ga:
            assert np.array_equal(ga[n].view(np.uint8), gb[n].view(np.uint8)), n
        a.playout(3, ids)
        assert a._sample_ticket == 5
        b.playout(3, ids, ticket=2)
        a.playout_boards_dev(dev, 4)
        assert a._sample_ticket == 9
        b.playout_boards_dev(dev, 4, ticket=5)
        SU.same(_state(a), _state(b), "ticket=None", np_lead=True)
        for call in (lambda: a.playout(0), lambda: a.playout(4097), lambda: a.playout(3, [1, 1]),
                     lambda: a.playout_boards_dev(torch.arange(33, dtype=torch.int32, device=a.device), 3)):
            with pytest.raises(_lib.TDError):
                call()
            assert a._sample_ticket == 9
        SU.same(_state(a), _state(b), "refused calls", np_lead=True)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------ 4: lists
def _poison(eng):
    eng._playout_prepare(1, 0, 0.0, 0.0, True)
    for t in eng._playout_buf.values():
        if t is not None:
            t.view(torch.uint8).fill_(0xA5)


def _unnamed_rows_kept(eng, named):
    rest = np.setdiff1d(np.arange(eng.B), named)
    for n, t in eng._playout_buf.items():
        if t is not None:
            rows = t.view(torch.uint8).cpu().numpy().reshape(eng.B, -1)[rest]
            assert (rows == 0xA5).all(), (n, rest[np.flatnonzero((rows != 0xA5).any(axis=1))[:4]])


@pytest.mark.parametrize("mode,dev", [("def", False), ("2p", True), ("atk", True), ("atk", False)])
def test_lists(mode, dev):
    """Random subsets, every board, one board, and (device) a count below cap with poison behind
    it.  Boards not named keep every byte: state, both streams, flags (the twin never touched
    them) and their output rows, pre-filled with 0xA5."""
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=23)
    a, b = _pair(10, 48, mode, cfg, hp, True)
    rng = np.random.RandomState(3)
    try:
        _phase_shift((a, b), 16, 23)
        lists = [rng.permutation(48)[:17], rng.permutation(48), np.array([31]), rng.permutation(48)[:5]]
        for i, ids in enumerate(lists):
            ids = ids.astype(np.int32)
            _poison(a)
            where = "list %s dev=%s #%d" % (mode, dev, i)
            if dev:
                cap = np.concatenate([ids, np.full(7, 0x7FFFFFF0, dtype=np.int32)]) if i == 3 else ids
                t = torch.from_numpy(cap[:48]).to(a.device)
                count = torch.tensor([len(ids)], dtype=torch.int32, device=a.device) if i == 3 else None
                st = torch.zeros(4, dtype=torch.int32, device=a.device)
                a._keep_status = st
                _check(a, b, 7, 10 * i, 0.3, 0.3, where, boards=ids, dev=(t, count), first=True, full_step=False)
            else:
                _check(a, b, 7, 10 * i, 0.3, 0.3, where, boards=ids, first=True, full_step=False)
            _unnamed_rows_kept(a, ids)
        assert a.list_errors()[0] == 0
        _full_step_equal(a, b, "lists %s" % mode, True)
        # an empty list launches nothing
        before = _state(a)
        a.playout(3, np.zeros(0, dtype=np.int32))
        if dev:
            a.playout_boards_dev(torch.zeros(0, dtype=torch.int32, device=a.device), 3)
        SU.same(_state(a), before, "empty list")
    finally:
        a.close()
        b.close()


def test_refused_lists_change_nothing():
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=23)
    a = _engine(10, 48, "2p", False, cfg, hp, True)
    try:
        for p in range(6):
            _drive((a,), np.arange(48), p)
        _poison(a)
        before = _state(a)
        dev = a.device
        bad = [(torch.tensor([3, 9, 3, 5], dtype=torch.int32, device=dev), None, _lib.LIST_TWICE),
               (torch.tensor([3, 48, 4], dtype=torch.int32, device=dev), None, _lib.LIST_RANGE),
               (torch.tensor([1, 2, 3], dtype=torch.int32, device=dev), torch.tensor([4], dtype=torch.int32, device=dev),
                _lib.LIST_BAD_COUNT)]
        a.list_errors()
        for ids, count, code in bad:
            st = torch.zeros(4, dtype=torch.int32, device=dev)
            a.playout_boards_dev(ids, 5, count=count, status=st, ticket=1, first=True)
            assert int(st.cpu()[0]) == code
            SU.same(_state(a), before, "refused %d" % code)
            _unnamed_rows_kept(a, np.zeros(0, dtype=np.int64))
        n, first = a.list_errors()
        assert n == 3 and first["code"] == _lib.LIST_TWICE
        # host refusals: nothing enqueued, whole messages
        for call, msg in ((lambda: a.playout(0), "steps = 0 outside [1, 4096]"),
                          (lambda: a.playout(4097), "steps = 4097 outside"),
                          (lambda: a.playout(3, [1, 1]), "td_playout_boards:"),
                          (lambda: a.playout(3, [48]), "td_playout_boards:")):
            with pytest.raises(_lib.TDError) as ei:
                call()
            assert msg in str(ei.value), str(ei.value)
        SU.same(_state(a), before, "host refusals")
    finally:
        a.close()


def test_refused_handles():
    """A multi-action handle and random_agent = 0 are refused, frame skip plays no part."""
    e = TDEngine(10, 4, "def", True, 1, np_seeds=np.arange(4) + 500, py_seeds=np.arange(4) + 500)
    try:
        with pytest.raises(_lib.TDError) as ei:
            e.playout(2)
        assert "multi-action" in str(ei.value)
    finally:
        e.close()
    e = TDEngine(10, 4, "def", False, 1, np_seeds=np.arange(4) + 500, py_seeds=np.arange(4) + 500, random_agent=False,
                 autoreset=False)
    try:
        with pytest.raises(_lib.TDError) as ei:
            e.playout(2)
        assert "random_agent = 0" in str(ei.value)
    finally:
        e.close()
    cfg, hp = M.config(M.RICH), M.hyper(max_episode_steps=23)
    a, b = _pair(10, 16, "def", cfg, hp, True)
    try:
        a.set_frame_skip(4)
        _check(a, b, 6, 0, 0, 0, "frame skip set", full_step=False)
        assert a._h and _lib.lib.td_frame_skip(a._h) == 4
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------- 5: the device-only loop
def test_device_only_search_loop():
    """Fork, step the chosen move and play out on device lists with no host copy, equal to the
    host-list twin."""
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=40)
    a, b = _pair(10, 48, "def", cfg, hp, True)
    try:
        for p in range(8):
            _drive((a, b), np.arange(48), p)
        src, dst = np.repeat(np.arange(4), 8).astype(np.int32), np.arange(16, 48, dtype=np.int32)
        dsrc, ddst = torch.from_numpy(src).to(a.device), torch.from_numpy(dst).to(a.device)
        for it in range(3):
            a.copy_boards_dev(dsrc, ddst)
            out = a.sample_actions_boards_dev(ddst, ticket=200 + it)
            a.step_boards_dev(ddst, def_act=out["def"])
            got = a.playout_boards_dev(ddst, 9, ticket=300 + 10 * it, def_idle=0.3)
            b.copy_boards(src, dst)
            out = b.sample_actions_boards(dst, ticket=200 + it)
            b.step_boards(dst, def_act=out["def"])
            want = _twin_loop(b, dst, 9, 300 + 10 * it, 0.3, 0.0)
            _same_outputs(got, want, dst, "search %d" % it)
            SU.same(_state(a), _state(b), "search %d" % it, np_lead=True)
        assert a.list_errors()[0] == 0
        _full_step_equal(a, b, "search", True)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------- 6: crowds
@pytest.mark.parametrize("mode,regime,seed", PR.CROWD_CASES)
def test_crowds(mode, regime, seed):
    """swarm / fortress configs against the twin; the floors are read from the twin's exports:
    past 64 live enemies (swarm), and at 32 towers (fortress)."""
    cfg, hp = PR.crowd_config(regime, seed)
    a, b = _pair(10, 16, mode, cfg, hp, True)
    try:
        top_en = top_tw = 0
        for r in range(PR.CROWD_ROUNDS):
            _check(a, b, 16, 16 * r, 0, 0, "crowd %s %s r=%d" % (mode, regime, r), full_step=False)
            hdr = b.export_state()["hdr"]
            top_en, top_tw = max(top_en, int(hdr["n_en"].max())), max(top_tw, int(hdr["n_tw"].max()))
        print("crowd %s %s: enemies %d towers %d" % (mode, regime, top_en, top_tw))
        if regime == "swarm":
            assert top_en > 64, top_en
        else:
            assert top_tw == 32, top_tw
        _full_step_equal(a, b, "crowd", True)
    finally:
        a.close()
        b.close()


# ----------------------------------------------------------------------- 7: never reset
def test_never_reset_boards():
    """Two failing seeds of the golden road table and two boards left out of reset(), among 16
    TD-2p boards: such a board gets reward 0, done 1, steps_run 0, the no-op and all 4 as its first
    actions and TD_FLAG_NO_LAYOUT; nothing else of it changes (its state bytes and both streams
    before and after, and the twin's)."""
    import goldens as G
    rows = G.load_roadgen()["10"]
    err = sorted(int(s) for s in rows if "err" in rows[s])[:2]
    good = sorted(int(s) for s in rows if "err" not in rows[s])[:14]
    seeds = np.array(sorted(err + good))
    left_out = [3, 11]
    assert len(err) == 2 and all(seeds[b] in good for b in left_out)
    failing = [b for b, s in enumerate(seeds) if s in err]
    never = np.array(sorted(failing + left_out))
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=23)
    engs = []
    try:
        for _ in range(2):
            e = TDEngine(10, 16, "2p", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, cfg=cfg, hp=hp,
                         sample_seed=SEED)
            mask = np.ones(16, dtype=np.uint8)
            mask[left_out] = 0
            _, failed = e.reset(mask)
            assert sorted(failed) == failing, (failed, failing)
            engs.append(e)
        a, b = engs
        st0 = a.export_state()
        assert (st0["hdr"]["num_roads"][never] == 0).all() and (st0["hdr"]["flags"] == 0).all()
        live = np.setdiff1d(np.arange(16), never)
        assert (st0["hdr"]["num_roads"][live] > 0).all()
        before = _state(a)
        _poison(a)
        got, _ = _check(a, b, 6, 0, 0, 0, "never reset", never=never, first=True, full_step=False)
        g = {n: v.cpu().numpy() for n, v in got.items() if v is not None}
        assert (g["reward"][never].view(np.uint64) == 0).all()  # +0.0
        assert (g["done"][never] == 1).all() and (g["steps_run"][never] == 0).all()
        assert (g["win"][never] == -1).all() and (g["allow_next"][never] == 0).all() and (g["cooldowns"][never] == 0).all()
        assert (g["ep_return"][never] == 0).all() and (g["ep_len"][never] == 0).all()
        assert (g["first_def"][never] == 600).all() and (g["first_atk"][never] == 4).all()
        assert (g["steps_run"][live] > 0).all()
        assert (a.flags()[never] == 8).all() and (a.flags()[live] == 0).all()
        after = _state(a)
        for k in before:  # nothing else of such a board changed
            if k not in ("flags", "np") and isinstance(before[k], np.ndarray) and before[k].shape[0] == 16:
                x, y = before[k][never].copy(), after[k][never].copy()
                if k == "state.hdr":  # the header's flag word (TdHdr word 18) is the one change
                    x[:, 72:76] = y[:, 72:76] = 0
                assert np.array_equal(x, y), k
        # again, with the flag already set, and then a full step of both engines
        _check(a, b, 6, 6, 0, 0, "never reset again", never=never, first=True)
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------------------ 8: config epochs
def test_config_change_between_playouts():
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=40)
    cfg2 = M.config(M.RICH, M.ATK, tower_cost=[[4, 9], [6, 11], [9, 14], [7, 12]], tower_attack=[[7, 9], [3, 4], [9, 12], [2, 3]],
                    enemy_LP=[[12, 22], [7, 12], [32, 52], [16, 26]])
    a, b = _pair(10, 32, "2p", cfg, hp, True)
    try:
        _check(a, b, 12, 0, 0.3, 0.3, "epoch 0", full_step=False)
        for e in (a, b):
            e.set_config(cfg2, hp)
        _check(a, b, 12, 12, 0.3, 0.3, "epoch 1", full_step=False)
        _check(a, b, 12, 24, 0.3, 0.3, "epoch 1 again")
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------- 9: TDVecEnv
def test_vec_env_playout_with_action_mask():
    v = E.TDVecEnv(10, 32, "2p", seed=500, action_mask=True)
    try:
        v.reset()
        ret, done, length = v.playout(9)
        assert ret.dtype == torch.float64 and done.dtype == torch.uint8 and length.dtype == torch.int32
        assert (length > 0).all() and ret.shape == (32,)
        kept = {k: t.clone() for k, t in v._masks.items()}  # what the playout left
        fresh = v.engine.action_mask()
        for k in kept:
            assert torch.equal(kept[k], fresh[k]), k
        ids = np.arange(3, 20, dtype=np.int32)
        v.playout(4, ids)
        kept = {k: t.clone() for k, t in v._masks.items()}  # what the playout left
        fresh = v.engine.action_mask()
        for k in kept:
            assert torch.equal(kept[k], fresh[k]), k
        v.playout_dev(torch.from_numpy(ids).to(v.engine.device), 4)
        kept = {k: t.clone() for k, t in v._masks.items()}  # what the playout left
        fresh = v.engine.action_mask()
        for k in kept:
            assert torch.equal(kept[k], fresh[k]), k
    finally:
        v.close()


# ---------------------------------------------------------------- 10: kernel name and timing
@pytest.mark.parametrize("L,mode,name", [(10, "def", "td_playout_kernel<10, 0>"), (20, "atk", "td_playout_kernel<20, 1>"),
                                         (12, "2p", "td_playout_kernel<0, 2>")])
def test_kernel_name_and_timing(L, mode, name):
    e = _engine(L, 8, mode, False, M.config(M.RICH, M.ATK), M.hyper(), True)
    try:
        assert e.playout_kernel_name() == name
        e.kernel_timing(4)
        e.playout(3)
        e.playout(3, [1, 2])
        e.playout_boards_dev(torch.tensor([4, 5], dtype=torch.int32, device=e.device), 3)
        t = e.kernel_times()
        assert len(t) == 3 and all(x > 0 for x in t), t
    finally:
        e.close()


# ------------------------------------------------------------------------ 11: a caller's stream
def test_on_a_lagging_stream():
    """Fork, step and play out on a caller's stream that lags behind the host, against the twin on
    the default stream."""
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=23)
    a, b = _pair(10, 48, "2p", cfg, hp, True)
    stream = torch.cuda.Stream()
    ahead = 0
    try:
        ids = np.arange(0, 48, 2, dtype=np.int32)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for r in range(4):
                SU.lag(stream)
                out = a.sample_actions(ticket=r)
                a.step(def_act=out["def"], atk_act=out["atk"])
                a.playout(6, ticket=100 + 10 * r, def_idle=0.3)
                a.playout(5, ids, ticket=200 + 10 * r, atk_idle=0.3)
                ahead += int(SU.ran_ahead(stream))
            stream.synchronize()
        for r in range(4):
            out = b.sample_actions(ticket=r)
            b.step(def_act=out["def"], atk_act=out["atk"])
            _twin_loop(b, np.arange(48), 6, 100 + 10 * r, 0.3, 0.0)
            _twin_loop(b, ids, 5, 200 + 10 * r, 0.0, 0.3)
        assert ahead > 0
        SU.same(_state(a), _state(b), "lagging stream", np_lead=True)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------ 12: oracle anchor
@pytest.mark.parametrize("case", PR.ANCHOR_CASES, ids=lambda c: c["name"])
def test_oracle_anchor(case):
    """The device against reference_playout on the CPU oracle itself (tests/playoutref.py)."""
    ref = PR.run_case(case)
    n = len(ref["seeds"])
    eng = TDEngine(case["L"], n, case["mode"], False, 1, np_seeds=ref["seeds"], py_seeds=ref["seeds"], autoreset=True,
                   cfg=ref["cfg"], hp=ref["hp"], sample_seed=PR.SAMPLE_SEED)
    try:
        _, failed = eng.reset()
        assert not failed
        for b in range(n):  # run_case's warm-up: board b starts b mod k sub-steps into its episode
            if b % case["k"]:
                eng.playout(b % case["k"], [b], ticket=PR.SHIFT_TICKET, def_idle=case["idle"], atk_idle=case["idle"])
        for r, ((k, ticket), want) in enumerate(zip(PR.round_plan(case), ref["rounds"])):
            got = {n_: v.cpu().numpy() for n_, v in eng.playout(k, ticket=ticket, def_idle=case["idle"],
                                                                atk_idle=case["idle"], first=True).items() if v is not None}
            for b in range(n):
                w = want[b]
                assert got["reward"][b].view(np.uint64) == np.float64(w["reward"]).view(np.uint64), (r, b, got["reward"][b], w["reward"])
                assert got["done"][b] == w["done"] and got["steps_run"][b] == w["steps_run"], (r, b)
                if w["first_def"] is not None:
                    assert got["first_def"][b] == w["first_def"], (r, b)
                if w["first_atk"] is not None:
                    assert np.array_equal(got["first_atk"][b], w["first_atk"]), (r, b)
        assert (eng.flags() == 0).all()
    finally:
        eng.close()
