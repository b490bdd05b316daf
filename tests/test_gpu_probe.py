"""Probes on the device (td_probe[_boards[_dev]] / TDEngine.probe*): `reps` random playouts per
board, the board left untouched.

Replica r of a probe is held, bit for bit, to its definition: a fresh twin engine with the same
seeds and call history on which ``playout(steps, boards, ticket + r * steps)`` is run
(tests/probeutil.py).  Beside the parity: nothing of the handle changes -- state, both streams down
to the raw words and the lazy-twist boundary, flags, episode statistics and records, every output
tensor of the step and the playout, the observation buffer and what the handle knows of it."""
import numpy as np
import pytest
import torch

import maskutil as M
import probeutil as PU
import streamutil as SU

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import envs as E  # noqa: E402
from gym_TD import sampling as S  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402

B = 12
LIMIT = 50  # max_episode_steps: boards stand 5 .. 49 steps into their episodes (probeutil.spread)
IDLE = 0.3


def _cfg(limit=LIMIT, **kw):
    return M.config(M.RICH, M.ATK, **kw), M.hyper(max_episode_steps=limit)


def _parity(L, mode, reps, steps, ticket, where, n=B, autoreset=True):
    """A probe of every board against its twins; returns the guards (probeutil.guards).  The base
    cannot fall, so every episode ends at the step limit and where the boards stand is known."""
    cfg, hp = _cfg(base_LP=10 ** 6)
    make = lambda: PU.engine(L, n, mode, cfg, hp, autoreset, PU.spread(LIMIT))  # noqa: E731
    rows = np.arange(n)
    want = PU.twins(make, steps, reps, None, ticket, IDLE, IDLE)
    eng = make()
    try:
        got = eng.probe(steps, reps, ticket=ticket, def_idle=IDLE, atk_idle=IDLE, first=True)
        for name in ("reward", "done", "steps_run", "win"):
            assert tuple(got[name].shape) == (n, reps), (name, got[name].shape)
        PU.same_rows(got, want, rows, where)
        assert (eng.flags() == 0).all()
    finally:
        eng.close()
    g = PU.guards(want, rows, reps)
    print("%s: done %d / %d, steps_run %s, replicas differ %s" % (where, int((want["done"] != 0).sum()), want["done"].size,
                                                                 np.bincount(want["steps_run"].reshape(-1)), g[2]))
    return g


# ------------------------------------------------------------------------------ 1: parity sweep
@pytest.mark.parametrize("mode", ["def", "atk", "2p"])
@pytest.mark.parametrize("reps", [1, 3])
@pytest.mark.parametrize("steps", [1, 6, 40])
def test_parity_sweep(mode, reps, steps):
    """12 boards of 10x10, episodes of 50 steps, the boards 5 .. 49 steps into theirs: some
    replicas end their episode and some do not, in every case; with three replicas some board's
    replicas differ in first action or return.  The ticket runs across the 2^64 wrap."""
    done, open_, differ = _parity(10, mode, reps, steps, S.M64 - 3, "sweep %s reps=%d steps=%d" % (mode, reps, steps))
    assert done and open_, (done, open_)
    assert differ or reps == 1


@pytest.mark.parametrize("L,mode", [(7, "def"), (20, "atk"), (30, "def")])
def test_parity_other_sizes(L, mode):
    """The generic build (7x7: hand-made layouts, no auto-reset), 20x20 and 30x30, in the modes that
    carry the private stream; three replicas of 40 sub-steps."""
    done, open_, differ = _parity(L, mode, 3, 40, 77, "L=%d %s" % (L, mode), autoreset=L != 7)
    assert done and open_ and differ, (done, open_, differ)


# -------------------------------------------------------------------------------- 2: stream wrap
def _drive_to_the_block_end(eng, need=3, lo=520, hi=616, most=600):
    """Ordinary steps until at least ``need`` boards' opponent streams stand in [lo, hi] of their
    624-word block; returns the number of steps (the same on every engine of these seeds)."""
    for t in range(most):
        if t % 4 == 0:
            pos = np.array([int(eng.get_py_state(b)[624]) for b in range(eng.B)])
            if t >= 8 and int(((pos >= lo) & (pos <= hi)).sum()) >= need:
                return t
        PU.full_steps(1, 7000 + t)(eng)
    raise AssertionError("no board's stream came near its block's end in %d steps" % most)


@pytest.mark.parametrize("mode", ["def", "atk"])
def test_stream_wrap(mode):
    """64 boards driven with ordinary steps until some opponent streams stand shortly before word
    624, then a probe of 48 sub-steps: in the twin at least one board's stream wraps into its next
    block during the playout (its position from td_get_py_state falls), and parity holds on every
    board -- the private copy twists lazily and wraps as the board's own stream would have."""
    n, steps, reps = 64, 48, 2
    cfg, hp = M.config(M.RICH, M.ATK, base_LP=10 ** 6), M.hyper()
    scout = PU.engine(10, n, mode, cfg, hp, True)
    try:
        drive = _drive_to_the_block_end(scout)
    finally:
        scout.close()
    make = lambda: PU.engine(10, n, mode, cfg, hp, True, PU.full_steps(drive))  # noqa: E731
    pos = {}

    def hook(r, eng, when):
        pos[(r, when)] = np.array([int(eng.get_py_state(b)[624]) for b in range(n)])

    want = PU.twins(make, steps, reps, None, 900, 0.0, 0.0, hook=hook)
    for r in range(reps):
        wrapped = np.flatnonzero(pos[(r, "after")] < pos[(r, "before")])
        print("wrap %s replica %d after %d steps: %d boards wrapped" % (mode, r, drive, len(wrapped)))
        assert len(wrapped) >= 1, (r, pos[(r, "before")], pos[(r, "after")])
    eng = make()
    try:
        before = PU.everything(eng)
        got = eng.probe(steps, reps, ticket=900, first=True)
        PU.same_rows(got, want, np.arange(n), "wrap %s" % mode)
        PU.unchanged(before, PU.everything(eng), "wrap %s" % mode)
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 3: nothing changes
def _poison_outputs(eng):
    """Every step and playout output tensor of the engine, every byte POISON (the observation is
    left as the last step wrote it)."""
    eng._playout_prepare(1, 0, 0.0, 0.0, True)
    for t in list(eng._playout_buf.values()) + [getattr(eng, n) for n in SU.OUTPUTS if n != "obs"]:
        if t is not None:
            t.view(torch.uint8).fill_(PU.POISON)


def _step_both(a, b, ticket):
    for e in (a, b):
        out = e.sample_actions(ticket=ticket, def_idle=IDLE, atk_idle=IDLE)
        e.step(def_act=out["def"], atk_act=out["atk"])


@pytest.mark.parametrize("mode,autoreset", [("def", True), ("atk", False), ("2p", True)])
def test_nothing_changes(mode, autoreset):
    """A retain_obs engine and a twin that never probes.  After a probe in which replicas finish
    episodes, every byte of probeutil.everything() is as before; the next step() of both engines
    gives equal outputs and equal observations.  Then the retained buffers of both are filled with
    poison: a probe in between or not, both engines' next steps skip the same windows -- the
    poison the twin's step leaves is left by the probed engine's too, so the probe did not touch
    what the handle knows of its buffer.  With auto-reset the engines then run on until every
    board has ended an episode and taken its next staged layout: the same layouts, so the probe
    moved no ring's head."""
    cfg, hp = _cfg()
    mk = lambda: PU.engine(10, B, mode, cfg, hp, autoreset, PU.spread(LIMIT), retain_obs=True)  # noqa: E731
    a, b = mk(), mk()
    try:
        _step_both(a, b, 100)  # (a full step: every board's observation is in the retained buffer)
        _poison_outputs(a)
        _poison_outputs(b)
        before = PU.everything(a)
        got = PU.host(a.probe(40, 3, ticket=5, def_idle=IDLE, atk_idle=IDLE, first=True))
        assert (got["done"] != 0).any() and (got["done"] == 0).any()  # replicas finished episodes, and not
        PU.unchanged(before, PU.everything(a), "probe %s" % mode)
        SU.same(SU.snapshot(a), SU.snapshot(b), "probed against never probed", np_lead=autoreset)
        _step_both(a, b, 101)
        SU.same(SU.snapshot(a), SU.snapshot(b), "the step after a probe", np_lead=autoreset)
        # the ledger: poison under both retained buffers, a probe on one engine, one step of both
        a.probe(6, 2, ticket=50)
        for e in (a, b):
            e.obs.view(torch.uint8).fill_(PU.POISON)
        a.probe(6, 2, [1, 5, 7], ticket=60)
        a.probe_boards_dev(torch.tensor([2, 3], dtype=torch.int32, device=a.device), 6, 2, ticket=70)
        _step_both(a, b, 102)
        oa, ob = a.obs.view(torch.uint8).cpu().numpy(), b.obs.view(torch.uint8).cpu().numpy()
        assert np.array_equal(oa, ob)
        kept = float((ob == PU.POISON).mean())
        print("nothing changes %s: %.1f %% of the retained buffer left unwritten by the next step" % (mode, 100 * kept))
        if a.retain_obs:  # (a step that wrote every byte would leave none)
            assert kept > 0.25, kept
        if autoreset:  # every board through an episode end: the next layouts are the twin's
            for t in range(LIMIT + 1):
                _step_both(a, b, 200 + t)
                if t % 10 == 3:
                    a.probe(5, 2, ticket=300 + t)
            assert (a.export_state()["hdr"]["episodes"] >= 1).all()
            SU.same(SU.snapshot(a), SU.snapshot(b), "after the episodes' ends", np_lead=True)
            assert (a.flags() == 0).all()
    finally:
        a.close()
        b.close()


# -------------------------------------------------------------------------------------- 4: lists
@pytest.mark.parametrize("mode", ["def", "2p"])
def test_lists(mode):
    """Host lists, device lists and a device list with a count below cap (poison ids behind it):
    the named boards' rows are the twins', every other board's [reps] rows keep their poison."""
    cfg, hp = _cfg()
    reps, steps = 3, 6
    make = lambda: PU.engine(10, B, mode, cfg, hp, True, PU.spread(LIMIT))  # noqa: E731
    rng = np.random.RandomState(3)
    lists = [rng.permutation(B)[:5].astype(np.int32), np.array([7], dtype=np.int32), rng.permutation(B).astype(np.int32)]
    eng = make()
    try:
        before = PU.everything(eng)
        for i, ids in enumerate(lists):
            want = PU.twins(make, steps, reps, ids, 40 + i, IDLE, IDLE)
            rest = np.setdiff1d(np.arange(B), ids)
            for form in ("host", "dev", "count"):
                out = PU.poison_probe(eng, reps)
                if form == "host":
                    got = eng.probe(steps, reps, ids, ticket=40 + i, def_idle=IDLE, atk_idle=IDLE, first=True)
                else:
                    cap = np.concatenate([ids, np.full(3, 0x7FFFFFF0, dtype=np.int32)])[:B] if form == "count" else ids
                    count = torch.tensor([len(ids)], dtype=torch.int32, device=eng.device) if form == "count" else None
                    got = eng.probe_boards_dev(torch.from_numpy(cap).to(eng.device), steps, reps, count=count,
                                               ticket=40 + i, def_idle=IDLE, atk_idle=IDLE, first=True)
                PU.same_rows(got, want, ids, "list %s #%d %s" % (mode, i, form))
                PU.rows_poisoned(out, rest)
        assert eng.list_errors()[0] == 0
        # an empty list launches nothing
        out = PU.poison_probe(eng, reps)
        eng.probe(steps, reps, np.zeros(0, dtype=np.int32))
        eng.probe_boards_dev(torch.zeros(0, dtype=torch.int32, device=eng.device), steps, reps)
        PU.rows_poisoned(out, np.arange(B))
        PU.unchanged(before, PU.everything(eng), "lists %s" % mode)
    finally:
        eng.close()


def test_refused_lists_write_nothing():
    cfg, hp = _cfg()
    eng = PU.engine(10, B, "2p", cfg, hp, True, PU.spread(LIMIT))
    try:
        out = PU.poison_probe(eng, 2)
        before = PU.everything(eng)
        dev = eng.device
        bad = [(torch.tensor([3, 9, 3, 5], dtype=torch.int32, device=dev), None, _lib.LIST_TWICE),
               (torch.tensor([3, B, 4], dtype=torch.int32, device=dev), None, _lib.LIST_RANGE),
               (torch.tensor([1, 2, 3], dtype=torch.int32, device=dev), torch.tensor([4], dtype=torch.int32, device=dev),
                _lib.LIST_BAD_COUNT)]
        eng.list_errors()
        for ids, count, code in bad:
            st = torch.zeros(4, dtype=torch.int32, device=dev)
            eng.probe_boards_dev(ids, 5, 2, count=count, status=st, ticket=1, first=True)
            assert int(st.cpu()[0]) == code
            PU.rows_poisoned(out, np.arange(B))
        n, first = eng.list_errors()
        assert n == 3 and first["code"] == _lib.LIST_TWICE
        # host refusals: nothing enqueued, whole messages, in the header's order
        for call, msg in ((lambda: eng.probe(0, 2), "td_probe: steps = 0 outside [1, 4096]"),
                          (lambda: eng.probe(4097, 0), "steps = 4097 outside"),
                          (lambda: eng.probe(3, 0), "td_probe: reps = 0 outside [1, 256] (TD_MAX_PROBE_REPS)"),
                          (lambda: eng.probe(3, -1, [1]), "td_probe_boards: reps = -1 outside"),
                          (lambda: eng.probe(3, 2, [1, 1]), "td_probe_boards:"),
                          (lambda: eng.probe(3, 2, [B]), "td_probe_boards:"),
                          (lambda: eng.probe_boards_dev(torch.arange(B + 1, dtype=torch.int32, device=dev), 3, 2),
                           "td_probe_boards_dev: cap = %d outside" % (B + 1))):
            with pytest.raises(_lib.TDError) as ei:
                call()
            assert msg in str(ei.value), str(ei.value)
        PU.rows_poisoned(out, np.arange(B))
        PU.unchanged(before, PU.everything(eng), "refused lists")
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 5: refused handles
def test_refused_handles():
    """A multi-action handle and random_agent = 0 are refused; a side the mode lacks is refused in
    front of both; frame skip plays no part."""
    seeds = np.arange(4) + 500
    e = TDEngine(10, 4, "def", True, 1, np_seeds=seeds, py_seeds=seeds)
    try:
        with pytest.raises(_lib.TDError) as ei:
            e.probe(2, 2)
        assert "td_probe: not supported with multi-action" in str(ei.value)
    finally:
        e.close()
    e = TDEngine(10, 4, "def", False, 1, np_seeds=seeds, py_seeds=seeds, random_agent=False, autoreset=False)
    try:
        with pytest.raises(_lib.TDError) as ei:
            e.probe(2, 2)
        assert "random_agent = 0" in str(ei.value)
        io, _, _ = e._probe_prepare(2, 2, 0, 0.0, 0.0, False)
        io.first_atk = io.reward  # (any non-NULL pointer: refused before anything is launched)
        assert _lib.lib.td_probe(e._h, io, None) < 0
        assert _lib.lib.td_last_error() == b"td_probe: TD-def has no attacker side (first_atk)"
        io.first_atk, io.done = None, None
        assert _lib.lib.td_probe(e._h, io, None) < 0
        assert _lib.lib.td_last_error() == b"td_probe: reward and done are required"
    finally:
        e.close()
    cfg, hp = _cfg()
    make = lambda: PU.engine(10, B, "def", cfg, hp, True, PU.spread(LIMIT))  # noqa: E731
    want = PU.twins(make, 6, 2, None, 0)
    e = make()
    try:
        e.set_frame_skip(4)
        PU.same_rows(e.probe(6, 2, ticket=0, first=True), want, np.arange(B), "frame skip set")
        assert _lib.lib.td_frame_skip(e._h) == 4
    finally:
        e.close()


# ------------------------------------------------------------------------- 6: never-reset boards
def test_never_reset_boards():
    """Two failing seeds of the golden road table and two boards left out of reset(), among 16
    TD-2p boards: every replica of such a board gets reward +0, done 1, steps_run 0, win -1, the
    no-op and all 4 as its first actions, and -- unlike the playout -- its header flag stays 0."""
    import goldens as G
    rows = G.load_roadgen()["10"]
    err = sorted(int(s) for s in rows if "err" in rows[s])[:2]
    good = sorted(int(s) for s in rows if "err" not in rows[s])[:14]
    seeds = np.array(sorted(err + good))
    left_out = [3, 11]
    failing = [b for b, s in enumerate(seeds) if s in err]
    never = np.array(sorted(failing + left_out))
    live = np.setdiff1d(np.arange(16), never)
    cfg, hp = _cfg(23)
    reps = 3

    def make():
        e = TDEngine(10, 16, "2p", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, cfg=cfg, hp=hp,
                     sample_seed=PU.SEED)
        mask = np.ones(16, dtype=np.uint8)
        mask[left_out] = 0
        _, failed = e.reset(mask)
        assert sorted(failed) == failing, (failed, failing)
        return e

    want = PU.twins(make, 6, reps, live, 0)
    eng = make()
    try:
        assert (eng.export_state()["hdr"]["num_roads"][never] == 0).all()
        PU.poison_probe(eng, reps)
        before = PU.everything(eng)
        got = eng.probe(6, reps, ticket=0, first=True)
        PU.same_rows(got, want, live, "never reset: the live boards")
        g = PU.host(got)
        assert (g["reward"][never].view(np.uint64) == 0).all()  # +0.0
        assert (g["done"][never] == 1).all() and (g["steps_run"][never] == 0).all() and (g["win"][never] == -1).all()
        assert (g["first_def"][never] == 600).all() and (g["first_atk"][never] == 4).all()
        assert (g["steps_run"][live] > 0).all()
        assert (eng.flags() == 0).all()  # TD_FLAG_NO_LAYOUT is not this call's to set
        PU.unchanged(before, PU.everything(eng), "never reset")
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 7: ticket counter
def test_ticket_none_takes_steps_times_reps():
    cfg, hp = _cfg()
    make = lambda: PU.engine(10, B, "2p", cfg, hp, True, PU.spread(LIMIT))  # noqa: E731
    t0 = S.M64 - 2  # (across the wrap)
    want = PU.twins(make, 5, 3, None, t0)
    a = make()
    try:
        a._sample_ticket = t0
        got = a.probe(5, 3, first=True)
        assert a._sample_ticket == (t0 + 15) & S.M64 == 12
        PU.same_rows(got, want, np.arange(B), "ticket=None")
        a.probe(5, 3, ticket=t0)
        assert a._sample_ticket == 12  # an explicit ticket leaves the counter alone
        a.probe(3, 2, [1, 4])
        assert a._sample_ticket == 18
        a.probe_boards_dev(torch.tensor([4, 5], dtype=torch.int32, device=a.device), 4, 4)
        assert a._sample_ticket == 34
        for call in (lambda: a.probe(0, 2), lambda: a.probe(4097, 2), lambda: a.probe(3, 0), lambda: a.probe(3, 257),
                     lambda: a.probe(3, 2, [1, 1]),
                     lambda: a.probe_boards_dev(torch.arange(B + 1, dtype=torch.int32, device=a.device), 3, 2)):
            with pytest.raises(_lib.TDError):
                call()
            assert a._sample_ticket == 34
    finally:
        a.close()


# ---------------------------------------------------------------------------------- 8: TDVecEnv
def test_vec_env_probe_with_action_mask():
    v = E.TDVecEnv(10, 32, "2p", seed=500, action_mask=True)
    try:
        v.reset()
        v.playout(9)  # (off the reset state; the masks are the playout's)
        kept = {k: t.clone() for k, t in v._masks.items()}
        serial = v.engine._state_serial
        ret, done, length = v.probe(9, 4)
        assert ret.dtype == torch.float64 and done.dtype == torch.uint8 and length.dtype == torch.int32
        assert ret.shape == done.shape == length.shape == (32, 4) and (length > 0).all()
        ids = np.arange(3, 20, dtype=np.int32)
        v.probe(4, 2, ids)
        v.probe_dev(torch.from_numpy(ids).to(v.engine.device), 4, 2)
        assert v.engine._state_serial == serial  # no state changed: nothing for a mask to go stale against
        for k in kept:  # the same tensors with the same bytes, and a fresh computation agrees
            assert torch.equal(v._masks[k], kept[k]), k
        fresh = v.engine.action_mask()
        for k in kept:
            assert torch.equal(kept[k], fresh[k]), k
    finally:
        v.close()


# ----------------------------------------------------------------------------- 9: lagging stream
def test_on_a_lagging_stream():
    """Steps and probes on a caller's stream that lags behind the host, against the twins on the
    default stream."""
    cfg, hp = _cfg()
    hist = PU.full_steps(3)
    make = lambda: PU.engine(10, B, "def", cfg, hp, True, hist)  # noqa: E731
    ids = np.arange(0, B, 2, dtype=np.int32)
    want_all = PU.twins(make, 6, 3, None, 100, IDLE)
    want_ids = PU.twins(make, 5, 2, ids, 200, IDLE)
    a = PU.engine(10, B, "def", cfg, hp, True)
    stream = torch.cuda.Stream()
    ahead = 0
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for r in range(3):
                SU.lag(stream)
                PU.full_steps(1, 7000 + r)(a)
                ahead += int(SU.ran_ahead(stream))
            SU.lag(stream)
            got_all = {n: (t.clone() if t is not None else None)
                       for n, t in a.probe(6, 3, ticket=100, def_idle=IDLE, first=True).items()}
            got_ids = a.probe(5, 2, ids, ticket=200, def_idle=IDLE, first=True)
            ahead += int(SU.ran_ahead(stream))
            stream.synchronize()
        assert ahead > 0
        PU.same_rows(got_all, want_all, np.arange(B), "lagging stream")
        PU.same_rows(got_ids, want_ids, ids, "lagging stream, list")
    finally:
        a.close()


# -------------------------------------------------------------------- 10: kernel name and timing
@pytest.mark.parametrize("L,mode,name", [(10, "def", "td_probe_kernel<10, 0>"), (20, "atk", "td_probe_kernel<20, 1>"),
                                         (12, "2p", "td_probe_kernel<0, 2>")])
def test_kernel_name_and_timing(L, mode, name):
    e = PU.engine(L, 8, mode, M.config(M.RICH, M.ATK), M.hyper(), True)
    try:
        assert e.probe_kernel_name() == name
        e.kernel_timing(4)
        e.probe(3, 2)
        e.probe(3, 2, [1, 2])
        e.probe_boards_dev(torch.tensor([4, 5], dtype=torch.int32, device=e.device), 3, 2)
        t = e.kernel_times()
        assert len(t) == 3 and all(x > 0 for x in t), t
    finally:
        e.close()
