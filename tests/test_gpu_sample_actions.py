"""Uniform legal-action sampling on the device (td_sample_actions[_boards[_dev]] /
TDEngine.sample_actions*).

* the kernel equals gym_TD.sampling.reference_sample over gym_TD.masks.reference_masks (both
  pinned to the CPU oracle: tests/test_sample_ref.py, tests/test_action_mask_ref.py) for every
  board, along runs driven by the sampler alone, across episode ends;
* the step is the judge: every sampled action was executed -- RealAction is the sampled action,
  FailCode 0;
* the idle edges, no side effect on any state, buffer edges and alignment, the list forms in both
  flavours with their refusals, degenerate boards, the fork / sample / step loop without a host
  copy, and a caller's stream.

An attacker summon counts as executed when its road's fail code is 0 and the first slot of
RealAction kept its type (tests/test_gpu_action_mask.py)."""
import numpy as np
import pytest
import torch

import maskutil as M
import sampleutil as U
import streamutil as SU
from oracle import policies

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import envs as E  # noqa: E402
from gym_TD import sampling as S  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402
from test_gpu_action_mask import _engine, _restart_7  # noqa: E402

# The sampler's seed.  Chosen among 1 .. 11 so that every case of the sampler-driven run reaches its
# floors: at L >= 30 a board's few level-ups stand among thousands of builds, and a uniform draw takes
# one about once in 120 steps of 8 or 16 boards (seeds 7, 9 and 11 do).
SEED = 7
MAXU = 2 ** 32 - 1
POISON64, POISON32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


def _host(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _step(eng, out):
    eng.step(def_act=out["def"], atk_act=out["atk"])


def _states(eng):
    st = eng.export_state()
    return [eng.board_state(b, st) for b in range(eng.B)], st


def _assert_equals_reference(eng, got, states, cfg, hp, ticket, def_idle, atk_idle, where, boards=None):
    ref = U.reference_batch(states, eng.L, cfg, hp, eng.mode, eng.multi, eng.sample_seed, ticket, def_idle, atk_idle, boards)
    for b, (d, a, dn, an) in ref.items():
        if eng.mode != "atk":
            assert np.array_equal(got["def"][b], d), (where, b, "def", got["def"][b] if not eng.multi else None, d if not eng.multi else None)
            assert got["def_count"][b] == dn, (where, b, "def_count", got["def_count"][b], dn)
        if eng.mode != "def":
            assert np.array_equal(got["atk"][b], a), (where, b, "atk", got["atk"][b], a)
            assert got["atk_count"][b] == an, (where, b, "atk_count", got["atk_count"][b], an)


# ------------------------------------------------- 1: the reference, and the step as judge
@pytest.mark.parametrize("mode,multi,L,B", [
    ("def", False, 10, 256), ("def", True, 10, 64), ("atk", False, 10, 64), ("2p", False, 20, 32),
    ("2p", True, 20, 32), ("def", False, 30, 16), ("def", False, 7, 32), ("def", False, 32, 8)])
def test_kernel_equals_reference_and_step_executes(mode, multi, L, B):
    """120 steps driven by the sampler alone (idle 0.3 on both sides, ticket = the step), auto-reset
    on, episodes of 60 steps.  Every step: what was sampled was executed.  Every 10th step:
    actions and counts of every board against the numpy reference on the exported state, and
    the counts against the sums of action_mask()'s rows.  (L = 7: caller layouts, the test
    restarts finished boards itself, as tests/test_gpu_action_mask.py.)  Multi-action TD-2p reports
    no attacker fail code (fail_atk is -1, as the reference's FailCode is None there): RealAction
    keeps the sampled type, and every 10th step the board is the judge -- cost_atk fell (every enemy costs more
    than a step's income) exactly on the boards that sampled a summon."""
    cfg = M.config(M.RICH) if mode == "def" else M.config(M.RICH, M.ATK)
    hp = M.hyper(multi, max_episode_steps=60)
    eng = _engine(L, B, mode, multi, cfg, hp, autoreset=True)
    eng.sample_seed = SEED
    NC = L * L
    try:
        seen = {"done": 0, "ops": np.zeros(6, dtype=int), "closed": 0, "def_idle": 0, "summons": 0, "atk_idle": 0, "paid": 0}
        for k in range(120):
            got = _host(eng.sample_actions(ticket=k, def_idle=0.3, atk_idle=0.3, counts=True))
            if k % 10 == 0:
                states, st = _states(eng)
                _assert_equals_reference(eng, got, states, cfg, hp, k, 0.3, 0.3, k)
                m = {n: v.cpu().numpy() for n, v in eng.action_mask().items()}
                if mode != "atk":
                    assert np.array_equal(got["def_count"], m["def"].reshape(B, -1)[:, :6 * NC].sum(axis=1)), k
                    live = (st["hdr"]["num_roads"] >= 1)
                    seen["closed"] += int(((st["hdr"]["def_cd"] > 1) & live).sum())
                    assert (got["def_count"][(st["hdr"]["def_cd"] > 1)] == 0).all(), k
                if mode != "def":
                    assert np.array_equal(got["atk_count"], m["atk"][:, :, :4].reshape(B, 12).sum(axis=1)), k
            _step(eng, eng._sample_buf)
            seen["done"] += int(eng.done.sum().item())
            if mode != "atk":
                rd = eng.real_def.cpu().numpy()
                assert np.array_equal(rd, got["def"]), (k, np.flatnonzero((rd != got["def"]).reshape(B, -1).any(axis=1))[:8])
                if multi:
                    flat = got["def"].reshape(B, -1)
                    assert (flat.sum(axis=1) <= 1).all() and ((flat == 0) | (flat == 1)).all(), k
                    picks = [int(np.flatnonzero(r)[0]) for r in flat if r.any()]
                else:
                    assert (eng.fail_def.cpu().numpy() == 0).all(), k
                    assert ((got["def"] >= 0) & (got["def"] <= 6 * NC)).all(), k
                    picks = [int(a) for a in got["def"] if a != 6 * NC]
                    seen["def_idle"] += int(((got["def"] == 6 * NC) & (got["def_count"] > 0)).sum())
                for a in picks:
                    seen["ops"][a // NC] += 1
            if mode != "def":
                ra, fa = eng.real_atk.cpu().numpy(), eng.fail_atk.cpu().numpy()
                for b in range(B):
                    rt = U.atk_pick(got["atk"][b])
                    if rt is not None and multi:  # no attacker fail code with multi-action (see the docstring)
                        assert ra[b, rt[0], 0] == rt[1] and (fa[b] == -1).all(), (k, b, rt, ra[b], fa[b])
                        seen["summons"] += 1
                    elif rt is not None:
                        assert ra[b, rt[0], 0] == rt[1] and fa[b, rt[0]] == 0, (k, b, rt, ra[b], fa[b])
                        seen["summons"] += 1
                    else:
                        seen["atk_idle"] += int(got["atk_count"][b] > 0)
            if mode == "2p" and multi and k % 10 == 0:  # the board as judge: a summon, and nothing else, lowers cost_atk
                after, _ = _states(eng)
                done = eng.done.cpu().numpy()
                for b in np.flatnonzero(done == 0):
                    summoned = U.atk_pick(got["atk"][b]) is not None
                    assert (after[b]["cost_atk"] < states[b]["cost_atk"]) == summoned, (k, b, states[b]["cost_atk"], after[b]["cost_atk"])
                    seen["paid"] += int(summoned)
            if L == 7:
                _restart_7(eng, np.flatnonzero(eng.done.cpu().numpy()))
        print("sampler run %s multi=%s L=%d B=%d: %r" % (mode, multi, L, B, seen))
        assert (eng.flags() == 0).all()
        assert seen["done"] > 0  # fresh episodes were sampled
        if mode != "atk":  # every branch of the defender's choice ran
            assert (seen["ops"][:4] > 0).all(), seen  # builds of all four tower types
            assert seen["ops"][4] > 0 and seen["ops"][5] > 0, seen  # a level-up and a destruct
            assert seen["closed"] > 0, seen  # boards with the cool-down closed were compared
        if mode != "def":
            assert seen["summons"] > 0, seen
            assert not (mode == "2p" and multi) or seen["paid"] > 0, seen
    finally:
        eng.close()


# ----------------------------------------------------------------------------- 2: idle edges
@pytest.fixture(scope="module")
def played():
    """A 64-board discrete TD-2p engine 25 sampler steps into the rich config."""
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper()
    eng = _engine(10, 64, "2p", False, cfg, hp, autoreset=True)
    eng.sample_seed = SEED
    for k in range(25):
        eng.sample_actions(ticket=k, def_idle=0.3, atk_idle=0.3)
        _step(eng, eng._sample_buf)
    yield eng, cfg, hp
    eng.close()


def test_idle_edges(played):
    eng, cfg, hp = played
    states, _ = _states(eng)
    got = _host(eng.sample_actions(ticket=100, def_idle=0, atk_idle=0, counts=True))
    assert (got["def_count"] > 0).any() and (got["atk_count"] > 0).any()
    assert (got["def"][got["def_count"] > 0] != 600).all()  # 0: nobody idles who could act
    assert all(U.atk_pick(a) is not None for a, n in zip(got["atk"], got["atk_count"]) if n > 0)
    _assert_equals_reference(eng, got, states, cfg, hp, 100, 0, 0, "idle 0")
    got = _host(eng.sample_actions(ticket=101, def_idle=MAXU, atk_idle=MAXU, counts=True))
    _assert_equals_reference(eng, got, states, cfg, hp, 101, MAXU, MAXU, "idle max")  # (not "all": u = 2^32 - 1 acts)
    for b in range(eng.B):
        if got["def_count"][b] > 0:
            assert (got["def"][b] == 600) == (S.u32(SEED, 101, b, S.DEF_IDLE) < MAXU), b
    # floats: 1.0 is 2^32 - 1 units, the same call
    again = _host(eng.sample_actions(ticket=101, def_idle=1.0, atk_idle=1.0, counts=True))
    assert all(np.array_equal(got[k], again[k]) for k in got)


# --------------------------------------------------------------- 3: nothing else is written
def test_sampling_writes_nothing_but_its_outputs():
    cfg, hp = M.config(M.RICH), M.hyper(max_episode_steps=30)
    a = _engine(10, 64, "def", False, cfg, hp, autoreset=True)
    b = _engine(10, 64, "def", False, cfg, hp, autoreset=True)
    try:
        rng = np.random.RandomState(7)

        def both(n):
            for _ in range(n):
                act = torch.from_numpy(np.array([policies.discrete_def(rng, 10) for _ in range(64)], dtype=np.int64))
                a.step(def_act=act)
                b.step(def_act=act)

        def state(e):
            st = {k: v.copy() for k, v in e.export_state().items()}
            st["flags"] = e.flags()
            for board in (0, 63):
                st["np%d" % board], st["py%d" % board] = e.get_np_state(board), e.get_py_state(board)
            return st

        both(35)  # (across an episode end)
        before = state(a)
        ids = torch.arange(0, 64, 3, dtype=torch.int32, device=a.device)
        a.sample_actions(def_idle=0.3, counts=True)
        a.sample_actions_boards(np.arange(5, 40, dtype=np.int32))
        a.sample_actions_boards_dev(ids, counts=True)
        after = state(a)
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        assert a._sample_ticket == 3  # each call took the engine's next ticket
        for k in range(10):  # the twin never sampled: the same bytes from the next step on
            both(1)
            a.sample_actions()
            assert np.array_equal(a.obs.cpu().numpy().view(np.uint32), b.obs.cpu().numpy().view(np.uint32)), k
            assert np.array_equal(a.reward.cpu().numpy().view(np.uint64), b.reward.cpu().numpy().view(np.uint64)), k
            assert np.array_equal(a.done.cpu().numpy(), b.done.cpu().numpy()), k
        sa, sb = a.export_state(), b.export_state()
        for name in sa:
            assert np.array_equal(sa[name], sb[name]), name
        assert not hasattr(a, "_mask_io")  # the sampler needs no mask buffer: action_mask was never called
    finally:
        a.close()
        b.close()


# ----------------------------------------------------------------------------- 4: buffer edges
def _raw(eng, ticket, def_act=None, atk_act=None, def_count=None, atk_count=None):
    io = _lib.TdSampleIO(def_act=def_act, atk_act=atk_act, def_count=def_count, atk_count=atk_count, seed=eng.sample_seed,
                         ticket=ticket, def_idle=U.IDLE_03, atk_idle=U.IDLE_03)
    rc = _lib.lib.td_sample_actions(eng._h, io, eng._stream())
    err = _lib.lib.td_last_error().decode() if rc < 0 else ""
    torch.cuda.synchronize()
    return rc, err


def _poisoned(n, dtype, front, device):
    """n elements behind `front` poisoned elements and in front of 16 more: (tensor, pointer, front)."""
    t = torch.full((front + n + 16,), POISON64 if dtype == torch.int64 else POISON32, dtype=dtype, device=device)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + front * t.element_size()


@pytest.mark.parametrize("front", [16, 17])  # def_act / atk_act at a multiple of 16, and of 8 only
def test_outputs_in_the_middle_of_a_larger_buffer(played, front):
    eng, _, _ = played
    B = eng.B
    want = _host(eng.sample_actions(ticket=7, def_idle=0.3, atk_idle=0.3, counts=True))
    bufs = {"def_act": _poisoned(B, torch.int64, front, eng.device), "atk_act": _poisoned(B * 24, torch.int64, front, eng.device),
            "def_count": _poisoned(B, torch.int32, front, eng.device), "atk_count": _poisoned(B, torch.int32, front, eng.device)}
    rc, err = _raw(eng, 7, **{k: p for k, (_, p) in bufs.items()})
    assert rc == 0, err
    for k, n, w in (("def_act", B, want["def"]), ("atk_act", B * 24, want["atk"]), ("def_count", B, want["def_count"]),
                    ("atk_count", B, want["atk_count"])):
        h = bufs[k][0].cpu().numpy()
        poison = POISON64 if h.dtype == np.int64 else POISON32
        assert (h[:front] == poison).all() and (h[front + n:] == poison).all(), k  # nothing in front of row 0, behind row B - 1
        assert np.array_equal(h[front:front + n], w.reshape(-1)), k


@pytest.mark.parametrize("front", [16, 17])
def test_multi_action_rows_at_both_alignments(front):
    """The [6][L][L] zero row is written whole in 16-B stores: the same values where def_act is a
    multiple of 8 but not of 16, and nothing outside the B rows (L = 7: rows of 294 elements)."""
    for L in (10, 7):
        cfg, hp = M.config(M.RICH), M.hyper(True)
        eng = _engine(L, 9, "def", True, cfg, hp, autoreset=True)
        try:
            eng.sample_seed = SEED
            for k in range(12):
                eng.sample_actions(ticket=k)
                _step(eng, eng._sample_buf)
            want = _host(eng.sample_actions(ticket=50, def_idle=0.3, counts=True))
            assert want["def"].any()
            n = eng.B * 6 * L * L
            t, p = _poisoned(n, torch.int64, front, eng.device)
            assert (p % 16 == 0) == (front == 16)
            rc, err = _raw(eng, 50, def_act=p)
            assert rc == 0, err
            h = t.cpu().numpy()
            assert (h[:front] == POISON64).all() and (h[front + n:] == POISON64).all(), L
            assert np.array_equal(h[front:front + n].reshape(want["def"].shape), want["def"]), L
        finally:
            eng.close()


def test_refusals_launch_nothing(played):
    eng, _, _ = played
    t, p = _poisoned(eng.B * 24, torch.int64, 16, eng.device)
    io = _lib.TdSampleIO(def_count=p)
    assert _lib.lib.td_sample_actions(eng._h, io, eng._stream()) < 0
    assert _lib.lib.td_last_error() == b"td_sample_actions: no action output wanted (def_act and atk_act are NULL)"
    cfg, hp = M.config(M.RICH), M.hyper()
    d = _engine(10, 4, "def", False, cfg, hp, autoreset=True)
    a = _engine(10, 4, "atk", False, M.config(M.ATK), hp, autoreset=True)
    try:
        for e, kw, word in ((d, dict(def_act=p, atk_act=p), "no attacker"), (d, dict(def_act=p, atk_count=p), "no attacker"),
                            (a, dict(atk_act=p, def_act=p), "no defender"), (a, dict(atk_act=p, def_count=p), "no defender")):
            rc, err = _raw(e, 0, **kw)
            assert rc < 0 and word in err, (kw, err)
        assert d.sample_actions()["atk"] is None and a.sample_actions()["def"] is None
    finally:
        d.close()
        a.close()
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == POISON64).all()


# ------------------------------------------------------------------------------ 5: list forms
LIST_B = 300


@pytest.fixture(scope="module")
def listed():
    """300 boards, 10x10 TD-2p discrete, at least 15 sampler steps in -- until the full call at ticket 9
    gives both sides something to do on some board; that call's rows."""
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper()
    eng = _engine(10, LIST_B, "2p", False, cfg, hp, autoreset=True)
    eng.sample_seed = SEED
    for k in range(40):
        eng.sample_actions(ticket=k, def_idle=0.3, atk_idle=0.3)
        _step(eng, eng._sample_buf)
        full = {n: v.clone() for n, v in eng.sample_actions(ticket=9, def_idle=0.3, atk_idle=0.3, counts=True).items()}
        if k >= 14 and (full["def"] != 600).any() and (full["atk"] != 4).any():
            break
    assert (full["def"] != 600).any() and (full["atk"] != 4).any()
    yield eng, full
    eng.close()


def _bufs(eng):
    return {k: t for k, t in eng._sample_buf.items() if t is not None}


def _poison(eng):
    for k, t in _bufs(eng).items():
        t.fill_(POISON64 if t.dtype == torch.int64 else POISON32)


def _bytes(eng):
    return {k: t.clone() for k, t in _bufs(eng).items()}


def _lists():
    rng = np.random.RandomState(3)
    return {"one": np.array([17]), "ends": np.array([299, 4, 0, 150, 77]), "131": rng.permutation(LIST_B)[:131],
            "all": rng.permutation(LIST_B)}


@pytest.mark.parametrize("which", ["one", "ends", "131", "all"])
def test_list_forms_write_the_named_rows_only(listed, which):
    """One id, five with both ends, 131 (a partial last workgroup among several) and all 300
    shuffled (n = B): the named rows are the full call's under the same seed and ticket, every
    other byte stays poison, and the device form gives the host form's bytes."""
    eng, full = listed
    ids = _lists()[which].astype(np.int32)
    named = np.zeros(LIST_B, dtype=bool)
    named[ids] = True
    kw = dict(ticket=9, def_idle=0.3, atk_idle=0.3, counts=True)
    _poison(eng)
    eng.sample_actions_boards(ids, **kw)
    host = _bytes(eng)
    for k, t in host.items():
        h, f = t.cpu().numpy(), full[k].cpu().numpy()
        assert np.array_equal(h[named], f[named]), (which, k)
        assert (h[~named] == (POISON64 if h.dtype == np.int64 else POISON32)).all(), (which, k)
    _poison(eng)
    eng.sample_actions_boards_dev(torch.from_numpy(ids).to(eng.device), **kw)
    for k, t in _bytes(eng).items():
        assert torch.equal(t, host[k]), (which, k)
    # count_dev shorter than cap, poison ids behind it: the first n entries alone
    n = max(1, len(ids) // 2)
    padded = np.concatenate([ids[:n], np.full(len(ids) - n + 3, 10 ** 6, dtype=np.int32)])[:LIST_B]
    count = torch.tensor([n], dtype=torch.int32, device=eng.device)
    status = torch.full((4,), -1, dtype=torch.int32, device=eng.device)
    _poison(eng)
    eng.sample_actions_boards_dev(torch.from_numpy(padded).to(eng.device), count=count, status=status, **kw)
    first = np.zeros(LIST_B, dtype=bool)
    first[ids[:n]] = True
    for k, t in _bytes(eng).items():
        h, f = t.cpu().numpy(), full[k].cpu().numpy()
        assert np.array_equal(h[first], f[first]) and (h[~first] == (POISON64 if h.dtype == np.int64 else POISON32)).all(), (which, k)
    assert status.cpu().numpy()[0] == 0
    assert eng.list_errors() == (0, None)


def test_refused_lists_write_nothing(listed):
    eng, _ = listed
    kw = dict(ticket=9, counts=True)
    eng.list_errors()
    _poison(eng)
    twice = torch.tensor([5, 9, 200, 9], dtype=torch.int32, device=eng.device)
    status = torch.zeros(4, dtype=torch.int32, device=eng.device)
    eng.sample_actions_boards_dev(twice, status=status, **kw)
    assert status.cpu().numpy()[0] == _lib.LIST_TWICE
    count = torch.tensor([4], dtype=torch.int32, device=eng.device)
    eng.sample_actions_boards_dev(torch.tensor([1, 2, 3], dtype=torch.int32, device=eng.device), count=count, status=status, **kw)
    assert status.cpu().numpy()[0] == _lib.LIST_BAD_COUNT
    for k, t in _bytes(eng).items():
        assert (t.cpu().numpy() == (POISON64 if t.dtype == torch.int64 else POISON32)).all(), k
    n, first = eng.list_errors()
    assert n == 2 and first["code"] == _lib.LIST_TWICE and first["board"] == 9
    # on the host, before anything is enqueued
    for bad, word in (([0, LIST_B], "td_sample_actions_boards"), ([-1], "td_sample_actions_boards"), ([3, 8, 3], "twice"),
                      (list(range(LIST_B)) + [0], "td_sample_actions_boards")):
        with pytest.raises(_lib.TDError) as e:
            eng.sample_actions_boards(np.asarray(bad, dtype=np.int32), **kw)
        assert word in str(e.value), (bad, str(e.value))
    with pytest.raises(_lib.TDError):
        eng.sample_actions_boards_dev(torch.zeros(LIST_B + 1, dtype=torch.int32, device=eng.device), **kw)
    eng.sample_actions_boards(np.zeros(0, dtype=np.int32), **kw)  # an empty list: nothing
    for k, t in _bytes(eng).items():
        assert (t.cpu().numpy() == (POISON64 if t.dtype == torch.int64 else POISON32)).all(), k
    assert eng.list_errors() == (0, None)
    assert eng.sample_actions_kernel_name() == "td_sample_kernel<10>"


# ----------------------------------------------------------------------- 6: degenerate boards
def test_board_never_reset():
    """A board whose reset failed (a failing seed of the golden road table): the no-op / all 4, counts 0."""
    import goldens as G
    rows = G.load_roadgen()["10"]
    err = sorted(int(s) for s in rows if "err" in rows[s])[0]
    ok = sorted(int(s) for s in rows if "err" not in rows[s])[:3]
    seeds = np.array([ok[0], err, ok[1], ok[2]])
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper()
    for multi in (False, True):
        eng = TDEngine(10, 4, "2p", multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, cfg=cfg, hp=M.hyper(multi),
                       sample_seed=SEED)
        try:
            _, failed = eng.reset()
            assert failed == [1]
            for t in range(20):
                got = _host(eng.sample_actions(ticket=t, counts=True))
                assert got["def_count"][1] == 0 and got["atk_count"][1] == 0 and (got["atk"][1] == 4).all()
                assert not got["def"][1].any() if multi else got["def"][1] == 600
            assert (got["def_count"][[0, 2, 3]] > 0).all() and (got["atk_count"][[0, 2, 3]] > 0).all()
            states, _ = _states(eng)
            _assert_equals_reference(eng, got, states, cfg, hp, 19, 0, 0, "never reset")
        finally:
            eng.close()


def test_full_tower_list_samples_level_up_or_destruct_only():
    """32 towers (the device's capacity): no build is a candidate."""
    cfg, hp = M.config(M.CAP), M.hyper()
    eng = _engine(10, 4, "def", False, cfg, hp, autoreset=False)
    eng.sample_seed = SEED
    try:
        full = 0
        for k in range(80):
            got = _host(eng.sample_actions(ticket=k, counts=True))
            st = eng.export_state()
            for b in np.flatnonzero(st["hdr"]["n_tw"] == 32):
                assert 400 <= got["def"][b] < 600 and 32 <= got["def_count"][b] <= 64, (k, b, got["def"][b])
                full += 1
            _step(eng, eng._sample_buf)
            assert (eng.fail_def.cpu().numpy() == 0).all() and np.array_equal(eng.real_def.cpu().numpy(), got["def"]), k
        assert full > 0 and (eng.flags() == 0).all()
    finally:
        eng.close()


def test_full_enemy_list_has_no_attacker_candidate():
    """128 live enemies: attacker count 0, the action all 4."""
    cfg, hp = M.config(M.CROWD), M.hyper()
    eng = _engine(10, 2, "atk", False, cfg, hp, autoreset=False)
    eng.sample_seed = SEED
    try:
        flood = torch.zeros((2, 3, 8), dtype=torch.int64)
        for _ in range(40):
            st = eng.export_state()
            if (st["hdr"]["n_en"] == 128).any():
                break
            eng.step(atk_act=flood)
        b = int(np.argmax(st["hdr"]["n_en"] == 128))
        assert st["hdr"]["n_en"][b] == 128 and st["hdr"]["atk_cd"][b] <= 1 and st["hdr"]["cost_atk"][b] >= 1
        got = _host(eng.sample_actions(ticket=0, counts=True))
        assert got["atk_count"][b] == 0 and (got["atk"][b] == 4).all()
    finally:
        eng.close()


# ------------------------------------------------------------- 7: the loop it was built for
def test_fork_sample_step_loop_without_a_host_copy():
    """512 envs: fork_dev of 8 roots into 64 boards each (the root and 63 copies),
    sample_actions_boards_dev, step_boards_dev, 20 times, ids and actions never on the host --
    byte-equal to a twin driven through the host-list forms with the same seed and tickets.
    (The opponent's stream is compared in CPython's form: the raw words depend on how far a
    kernel has carried its lazy twist, and the host list runs another step kernel.)"""
    B, ROOTS = 512, 8
    src = np.repeat(np.arange(ROOTS), 63).astype(np.int32)
    dst = np.arange(ROOTS, B, dtype=np.int32)
    order = np.random.RandomState(11).permutation(B).astype(np.int32)
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper(max_episode_steps=15)

    def make():
        v = E.TDVecEnv(10, B, "2p", seed=40, sample_seed=SEED)
        v.engine.set_config(cfg, hp)  # (money and cool-downs: both sides act throughout; episodes end inside the run)
        v.reset()
        return v

    dev, host = make(), make()
    try:
        d_src, d_dst, d_all = (torch.from_numpy(x).to(dev.engine.device) for x in (src, dst, order))
        acted = torch.zeros(2, dtype=torch.int64, device=dev.engine.device)
        for it in range(20):
            dev.fork_dev(d_src, d_dst)
            act = dev.sample_actions_boards_dev(d_all, ticket=it, def_idle=0.3, atk_idle=0.3)
            dev.step_boards_dev(d_all, act)
            acted += torch.stack([(dev.engine.real_def != 600).sum(), dev.engine.done.sum()])
            host.fork(src, dst)
            act = host.sample_actions_boards(order, ticket=it, def_idle=0.3, atk_idle=0.3)
            host.step_boards(order, act)
        assert dev.engine.list_errors() == (0, None)
        a = SU.snapshot(dev.engine, extra=_bufs(dev.engine))
        b = SU.snapshot(host.engine, extra=_bufs(host.engine))
        a.pop("state.opp_mt"), b.pop("state.opp_mt")
        SU.same(a, b, "after 20 iterations", np_lead=True)
        acted = acted.cpu().numpy()
        assert acted[0] > 0 and acted[1] > 0 and (dev.engine.flags() == 0).all(), acted
    finally:
        dev.close()
        host.close()


# ---------------------------------------------------------------------- 8: a caller's stream
def test_on_a_callers_stream():
    """64 boards sampled and stepped inside torch.cuda.stream(S), S lagging behind the host: the
    outputs and states of a twin on the default stream."""
    cfg, hp = M.config(M.RICH, M.ATK), M.hyper()
    S_ = torch.cuda.Stream()
    snaps = []
    for stream in (S_, None):
        eng = _engine(10, 64, "2p", False, cfg, hp, autoreset=True)
        eng.sample_seed = SEED
        try:
            ids = torch.arange(0, 64, 2, dtype=torch.int32, device=eng.device)
            torch.cuda.synchronize()

            def run():
                for k in range(12):
                    if stream is not None and k % 4 == 0:
                        SU.lag(stream)
                    if k % 3 == 2:
                        eng.sample_actions_boards_dev(ids, ticket=k, def_idle=0.3, atk_idle=0.3, counts=True)
                        eng.step_boards_dev(ids, eng._sample_buf["def"], eng._sample_buf["atk"])
                    else:
                        eng.sample_actions(ticket=k, def_idle=0.3, atk_idle=0.3, counts=True)
                        _step(eng, eng._sample_buf)

            if stream is None:
                run()
            else:
                with torch.cuda.stream(stream):
                    run()
                    ahead = SU.ran_ahead(stream)
                    stream.synchronize()
                assert ahead  # the host had issued everything before the stream got there
            torch.cuda.synchronize()
            snaps.append(SU.snapshot(eng, extra=_bufs(eng)))
        finally:
            eng.close()
    SU.same(snaps[0], snaps[1], "caller's stream", np_lead=True)
