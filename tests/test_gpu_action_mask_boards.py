"""Legal-action masks for a named list of boards (td_action_mask_boards and
td_action_mask_boards_dev; TDEngine.action_mask_boards[_dev]; TDVecEnv's partial refresh).

The truth is td_action_mask on the same state (itself pinned to gym_TD/masks.py, to brute
force on the oracle and to the step by tests/test_gpu_action_mask.py).  Method of every byte
comparison: boards some tens of mask-policy steps into a rollout; the outputs are filled with a
sentinel (0xA5); the list call runs; then every byte of every output -- guard bytes in front
and behind included -- must equal the sentinel, except the rows of the named boards, which
must equal the rows the full call wrote into buffers laid out the same way."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import maskutil as M
from oracle import canon
from oracle import policies

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import envs as E  # noqa: E402
from gym_TD import params as P  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402
from gym_TD.masks import reference_masks  # noqa: E402

SENT, GUARD = 0xA5, 64
OK, BAD_COUNT, RANGE, TWICE = _lib.LIST_OK, _lib.LIST_BAD_COUNT, _lib.LIST_RANGE, _lib.LIST_TWICE
DEV = torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------ engines some tens of steps in
def _engine(L, B, mode, multi, cfg, hp, seed0=500, **kw):
    seeds = np.arange(B) + seed0
    if L == 7:  # no 7x7 map can be drawn: caller layouts (maskutil.hand_layouts_7)
        eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, cfg=cfg, hp=hp, **kw)
        recs = M.hand_layouts_7()
        eng.reset_layouts(np.stack([recs[b % 2] for b in range(B)]), np.arange(B))
        return eng
    kw.setdefault("autoreset", True)
    eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, cfg=cfg, hp=hp, **kw)
    eng.reset_all()
    return eng


def _play(eng, steps, seed=1000):
    """`steps` steps of maskutil's policy, which samples from the full call's masks."""
    L, mode, multi = eng.L, eng.mode, eng.multi
    rngs = [np.random.RandomState(seed + s) for s in range(eng.B)]
    for _ in range(steps):
        m = {k: v.cpu().numpy() for k, v in eng.action_mask().items()}
        da = aa = None
        if mode != "atk":
            da = np.stack([np.asarray(M.def_action(M.pick_def(r, row, L * L), L, multi), dtype=np.int64)
                           for r, row in zip(rngs, m["def"])])
        if mode != "def":
            aa = np.stack([M.atk_action(M.pick_atk(r, row)) for r, row in zip(rngs, m["atk"])])
        eng.step(def_act=None if da is None else torch.from_numpy(da), atk_act=None if aa is None else torch.from_numpy(aa))
    torch.cuda.synchronize()
    return eng


def _random_steps(eng, steps, seed):
    """`steps` steps of uniformly random discrete defender actions (large batches)."""
    rng = np.random.RandomState(seed)
    A = 6 * eng.L * eng.L + 1
    for _ in range(steps):
        eng.step(def_act=torch.from_numpy(rng.randint(0, A, size=eng.B).astype(np.int64)))
    torch.cuda.synchronize()
    return eng


@pytest.fixture(scope="module")
def def10():
    eng = _play(_engine(10, 37, "def", False, M.config(M.RICH), M.hyper()), 40)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def twop7():
    eng = _play(_engine(7, 9, "2p", False, M.config(M.RICH, M.ATK), M.hyper()), 30)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def twop20m():
    eng = _play(_engine(20, 6, "2p", True, M.config(M.RICH, M.ATK), M.hyper(True)), 30)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def atk10():
    eng = _play(_engine(10, 21, "atk", False, M.config(M.ATK), M.hyper()), 40)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def def30():
    eng = _play(_engine(30, 5, "def", False, M.config(M.RICH), M.hyper()), 30)
    yield eng
    eng.close()


# ------------------------------------------------------------------ buffers and the comparison
class Bufs(object):
    """One set of outputs: each a 16-B-aligned allocation of 16 + off + B * row + GUARD bytes,
    the output at byte 16 + off."""

    def __init__(self, eng, outs, pitch=0, off=None):
        off = off or {}
        self.eng, self.pitch, self.t, self.off, self.row = eng, pitch, {}, {}, {}
        NC = eng.L * eng.L
        for k in outs:
            self.row[k] = 15 if k == "atk" else (pitch or 6 * NC + (0 if eng.multi else 1))
            self.off[k] = 16 + off.get(k, 0)
            n = self.off[k] + eng.B * self.row[k] + GUARD
            self.t[k] = torch.full((n,), SENT, dtype=torch.uint8, device=eng.device)
            assert self.t[k].data_ptr() % 16 == 0

    def io(self):
        p = {k: self.t[k].data_ptr() + self.off[k] for k in self.t}
        return _lib.TdMaskIO(def_mask=p.get("def"), def_code=p.get("def_code"), atk_mask=p.get("atk"),
                             def_pitch=self.pitch)

    def host(self):
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in self.t.items()}

    def rows(self, k, h=None):
        """Output k as [B][row] (a view of the host copy h, or a fresh one)."""
        h = self.host()[k] if h is None else h
        return h[self.off[k]:self.off[k] + self.eng.B * self.row[k]].reshape(self.eng.B, self.row[k])


def _ids32(ids):
    return np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))


def _dev(ids):
    return torch.as_tensor(_ids32(ids)).to(DEV)


def _status():
    return torch.full((4,), -7, dtype=torch.int32, device=DEV)


def _full(eng, bufs):
    rc = _lib.lib.td_action_mask(eng._h, bufs.io(), eng._stream())
    assert rc == 0, _lib.lib.td_last_error()
    return bufs


def _host_call(eng, bufs, ids):
    a = _ids32(ids)
    rc = _lib.lib.td_action_mask_boards(eng._h, bufs.io(), a.ctypes.data if a.size else None, int(a.size), eng._stream())
    err = _lib.lib.td_last_error().decode() if rc < 0 else ""
    a[...] = -1  # the caller's array is free on return
    return rc, err


def _dev_call(eng, bufs, ids, count=None, status=None):
    t = ids if isinstance(ids, torch.Tensor) else _dev(ids)
    c = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
    rc = _lib.lib.td_action_mask_boards_dev(eng._h, bufs.io(), t.data_ptr() if t.numel() else None,
                                            int(t.numel()),
                                            c.data_ptr() if c is not None else None,
                                            status.data_ptr() if status is not None else None, eng._stream())
    err = _lib.lib.td_last_error().decode() if rc < 0 else ""
    torch.cuda.synchronize()  # (t and c stay alive until the kernels have run)
    return rc, err


def _assert_only(bufs, truth, named, where):
    """Every byte of bufs is the sentinel, except the rows of `named`: those are truth's."""
    got, want = bufs.host(), truth.host()
    for k in got:
        exp = np.full_like(got[k], SENT)
        r, o = bufs.row[k], bufs.off[k]
        for b in named:
            exp[o + b * r:o + (b + 1) * r] = want[k][o + b * r:o + (b + 1) * r]
        bad = np.flatnonzero(got[k] != exp)
        assert bad.size == 0, (where, k, "first differing byte %d (row %d)" % (bad[0], (bad[0] - o) // r), len(bad))


def _assert_clean(bufs, where):
    for k, h in bufs.host().items():
        assert (h == SENT).all(), (where, k)


def _lists(B, seed=5):
    """The lists every shape is run with (the kernel has four list entries per workgroup):
    n = 1; two adjacent ids, then the ids on either side of them in a second call into the same
    buffers; n = 3 and n = 5 (a partial last workgroup alone, and behind a full one); a random
    subset; a permutation of all B.  Each item: the calls' lists, in order."""
    rng = np.random.RandomState(seed)
    k = B // 2
    sub = rng.permutation(B)[:max(2, (2 * B) // 3)].tolist()
    return [("one", [[k]]), ("first", [[0]]), ("last", [[B - 1]]),
            ("adjacent, then either side", [[k, k + 1], [k + 2, k - 1]]),
            ("three", [[B - 1, 0, k]]), ("five", [[1, 0, 2, B - 1, B - 2]]),
            ("subset", [sub]), ("permutation", [rng.permutation(B).tolist()])]


def _run_lists(eng, outs, pitch=0, off=None, forms=("host", "dev")):
    truth = _full(eng, Bufs(eng, outs, pitch, off))
    for form in forms:
        for name, calls in _lists(eng.B):
            bufs, named = Bufs(eng, outs, pitch, off), []
            for ids in calls:
                rc, err = _host_call(eng, bufs, ids) if form == "host" else _dev_call(eng, bufs, ids)
                assert rc == 0, (form, name, err)
                named += ids
                _assert_only(bufs, truth, named, (form, name, len(named), pitch, off))
    if "dev" in forms:
        assert eng.list_errors() == (0, None)


# ------------------------------------------------------------------ 1. shapes x lists
@pytest.mark.parametrize("pitch,off_mask,off_code", [
    (0, 0, 0), (0, 1, 1), (0, 8, 8), (0, 0, 8), (0, 1, 0),  # 601: rows share 16-B pieces with their neighbours
    (608, 0, 0), (608, 1, 1), (608, 8, 0), (640, 0, 0), (640, 8, 8), (640, 1, 8)])
def test_def_10x10_pitch_and_alignment(def10, pitch, off_mask, off_code):
    """TD-def 10x10, B = 37: mask and code at byte offsets 0, 1 and 8 of a 16-B grid, together
    and apart (apart: the per-byte path of differently aligned outputs)."""
    _run_lists(def10, ("def", "def_code"), pitch, {"def": off_mask, "def_code": off_code})


@pytest.mark.parametrize("outs", [("def",), ("def_code",)])
@pytest.mark.parametrize("pitch,off", [(0, 0), (0, 1), (608, 0), (640, 8)])
def test_def_10x10_one_output_alone(def10, outs, pitch, off):
    _run_lists(def10, outs, pitch, {outs[0]: off})


def test_2p_7x7_generic_side_odd_cell_count(twop7):
    """TD-2p 7x7 on hand layouts, B = 9: the generic-L kernel, NC = 49, the per-cell path; rows of
    295 bytes and the 15-B attacker rows."""
    _run_lists(twop7, ("def", "def_code", "atk"))
    _run_lists(twop7, ("def", "atk"), 0, {"def": 1, "atk": 1}, forms=("host",))


@pytest.mark.parametrize("off", [0, 4])
def test_2p_20x20_multi_action(twop20m, off):
    """TD-2p 20x20 multi-action, B = 6: rows [6][L][L]."""
    _run_lists(twop20m, ("def", "def_code", "atk"), 0, {"def": off, "def_code": off})


@pytest.mark.parametrize("off", [0, 1])
def test_atk_10x10_every_line_shared(atk10, off):
    """TD-atk 10x10, B = 21: 15-B rows, eight boards and more to a 128-B line."""
    _run_lists(atk10, ("atk",), 0, {"atk": off})


def test_def_30x30(def30):
    _run_lists(def30, ("def", "def_code"))
    _run_lists(def30, ("def",), 5408, {"def": 8}, forms=("host",))


def test_many_workgroups_last_one_partial():
    """B = 1,031 TD-def boards, n = 1,000 scattered ids (a prime stride): 250 workgroups, in the
    device form with count = 998 the last one partial."""
    B = 1031
    eng = _random_steps(_engine(10, B, "def", False, M.config(M.RICH), M.hyper()), 30, 9)
    try:
        ids = [(i * 397 + 11) % B for i in range(1000)]
        assert len(set(ids)) == 1000
        outs = ("def", "def_code")
        truth = _full(eng, Bufs(eng, outs))
        bufs = Bufs(eng, outs)
        rc, err = _host_call(eng, bufs, ids)
        assert rc == 0, err
        _assert_only(bufs, truth, ids, "host")
        bufs = Bufs(eng, outs)
        rc, err = _dev_call(eng, bufs, ids, count=998)
        assert rc == 0, err
        _assert_only(bufs, truth, ids[:998], "dev")
        assert eng.list_errors() == (0, None)
    finally:
        eng.close()


def test_named_rows_equal_the_numpy_reference(def10):
    """The named rows against gym_TD/masks.py directly, not through the full call."""
    eng, cfg, hp = def10, M.config(M.RICH), M.hyper()
    ids = [31, 2, 3, 17, 36]
    bufs = Bufs(eng, ("def", "def_code"))
    rc, err = _host_call(eng, bufs, ids)
    assert rc == 0, err
    h = bufs.host()
    dm, dc = bufs.rows("def", h["def"]), bufs.rows("def_code", h["def_code"])
    st = eng.export_state()
    for b in ids:
        wm, wc, _ = reference_masks(eng.board_state(b, st), eng.L, cfg, hp, eng.mode, eng.multi)
        assert np.array_equal(dm[b], wm) and np.array_equal(dc[b], wc), b
    assert dm[ids, :-1].any() and dc[ids].any()


def test_never_reset_board_has_only_the_always_legal_entries():
    import goldens as G
    rows = G.load_roadgen()["10"]
    err = sorted(int(s) for s in rows if "err" in rows[s])[0]
    good = sorted(int(s) for s in rows if "err" not in rows[s])[:5]
    seeds = good[:2] + [err] + good[2:]
    eng = TDEngine(10, 6, "2p", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, cfg=M.config(M.RICH, M.ATK))
    try:
        _, failed = eng.reset()
        assert failed == [2]
        outs = ("def", "def_code", "atk")
        truth = _full(eng, Bufs(eng, outs))
        for form in ("host", "dev"):
            bufs = Bufs(eng, outs)
            rc, msg = (_host_call if form == "host" else _dev_call)(eng, bufs, [3, 2])
            assert rc == 0, msg
            _assert_only(bufs, truth, [3, 2], form)
            h = bufs.host()
            d, a = bufs.rows("def", h["def"]), bufs.rows("atk", h["atk"]).reshape(-1, 3, 5)
            assert d[2, -1] == 1 and not d[2, :-1].any()
            assert (a[2, :, 4] == 1).all() and not a[2, :, :4].any()
            assert d[3, :-1].any()  # (the board beside it was reset and can build)
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. the calls change nothing
def test_list_masks_do_not_change_the_step():
    """Two engines on the same seeds, one calling both list forms after every step: 40 steps of
    equal observations, rewards and dones, equal state digests, and td_kernel_times counts the
    steps alone."""
    cfg, hp = M.config(M.RICH), M.hyper(max_episode_steps=30)
    a = _engine(10, 64, "def", False, cfg, hp)
    b = _engine(10, 64, "def", False, cfg, hp)
    try:
        rng = np.random.RandomState(7)
        lrng = np.random.RandomState(8)
        a.kernel_timing(256)
        b.kernel_timing(256)
        for k in range(40):
            act = np.array([policies.discrete_def(rng, 10) for _ in range(64)], dtype=np.int64)
            a.step(def_act=torch.from_numpy(act))
            b.step(def_act=torch.from_numpy(act))
            ids = lrng.permutation(64)[:int(lrng.randint(1, 40))]
            b.action_mask_boards(ids, code=True)
            b.action_mask_boards_dev(_dev(ids[::-1].copy()), code=True)
            assert np.array_equal(a.obs.cpu().numpy().view(np.uint32), b.obs.cpu().numpy().view(np.uint32)), k
            assert np.array_equal(a.reward.cpu().numpy().view(np.uint64), b.reward.cpu().numpy().view(np.uint64)), k
            assert np.array_equal(a.done.cpu().numpy(), b.done.cpu().numpy()), k
        torch.cuda.synchronize()
        assert len(a.kernel_times()) == 40 and len(b.kernel_times()) == 40
        sa, sb = a.export_state(), b.export_state()
        for name in sa:
            assert np.array_equal(sa[name], sb[name]), name
        for i in range(64):
            assert canon.state_digest(a.board_state(i, sa)) == canon.state_digest(b.board_state(i, sb)), i
        assert (a.flags() == b.flags()).all()
        assert b.list_errors() == (0, None)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 3. the device form
def test_device_form_count_and_garbage_past_the_count(def10):
    eng = def10
    outs = ("def", "def_code")
    truth = _full(eng, Bufs(eng, outs))
    ids = [30, 4, 5, 6, 21, 0, 36]
    # count NULL: every entry
    bufs, st = Bufs(eng, outs), _status()
    rc, err = _dev_call(eng, bufs, ids, status=st)
    assert rc == 0, err
    _assert_only(bufs, truth, ids, "count NULL")
    assert st.tolist()[0] == OK and st.tolist()[2:] == [-1, -1]
    # count inside (0, cap), the entries past it garbage: out of range, negative, a board twice
    junk = ids[:5] + [eng.B + 1000, -3, ids[0], 2 ** 31 - 1]
    bufs, st = Bufs(eng, outs), _status()
    rc, err = _dev_call(eng, bufs, junk, count=5, status=st)
    assert rc == 0, err
    _assert_only(bufs, truth, ids[:5], "count 5 of 9")
    assert st.tolist()[0] == OK
    # count = cap
    bufs = Bufs(eng, outs)
    rc, err = _dev_call(eng, bufs, ids, count=len(ids))
    assert rc == 0, err
    _assert_only(bufs, truth, ids, "count = cap")
    # count = 0: nothing is written, the status is OK
    bufs, st = Bufs(eng, outs), _status()
    rc, err = _dev_call(eng, bufs, junk, count=0, status=st)
    assert rc == 0, err
    _assert_clean(bufs, "count 0")
    assert st.tolist()[0] == OK
    # an int64 list through the engine: converted on the device
    eng.action_mask(code=True)
    m = eng.action_mask_boards_dev(torch.tensor(ids, dtype=torch.int64, device=DEV), code=True)
    assert torch.equal(m["def"], truth_rows(truth, "def")) and torch.equal(m["def_code"], truth_rows(truth, "def_code"))
    assert eng.list_errors() == (0, None)


def truth_rows(truth, k):
    A = 6 * truth.eng.L * truth.eng.L + 1
    return torch.from_numpy(truth.rows(k)[:, :A].copy()).to(DEV)


def test_device_refusals_write_nothing():
    """A bad count, an id = B, an id = -1 and a board twice: every byte stays the sentinel,
    status_dev shows code / entry / board, the serial advances by one per launched call (a
    td_step_boards_dev call in between takes one too), td_list_errors counts them."""
    eng = _play(_engine(10, 16, "def", False, M.config(M.RICH), M.hyper(), seed0=540), 10)
    try:
        B, outs = eng.B, ("def", "def_code")
        truth = _full(eng, Bufs(eng, outs))
        assert eng.list_errors() == (0, None)
        cases = [  # ids, count, code, entries, board
            ([1, 2, 3], 4, BAD_COUNT, {-1}, 4),
            ([1, 2, 3], -1, BAD_COUNT, {-1}, -1),
            ([3, B, 5], None, RANGE, {1}, B),
            ([3, 4, 5, -1], None, RANGE, {3}, -1),
            ([5, 6, 7, 8, 5], None, TWICE, {0, 4}, 5),
        ]
        serial = 0
        for ids, count, code, entries, board in cases:
            tag = (ids, count)
            bufs, st = Bufs(eng, outs), _status()
            rc, err = _dev_call(eng, bufs, ids, count=count, status=st)
            assert rc == 0, (tag, err)  # the call itself is accepted: the device refuses
            _assert_clean(bufs, tag)
            got = st.tolist()
            assert got[0] == code and got[1] == serial and got[2] in entries and got[3] == board, (tag, got)
            n, first = eng.list_errors()
            assert n == 1 and first == dict(code=code, call=serial, entry=got[2], board=board), (tag, n, first)
            serial += 1
            # a step's device list in between takes the next serial (the pass: a legal no-op action)
            st = _status()
            eng.step_boards_dev(_dev([0, 9]), def_act=torch.full((B,), 600, dtype=torch.int64), status=st)
            torch.cuda.synchronize()
            assert st.tolist() == [OK, serial, -1, -1], (tag, st.tolist())
            serial += 1
            # and the valid list of the same boards works right behind the refusal
            truth = _full(eng, Bufs(eng, outs))
            good = sorted(set(i for i in ids if 0 <= i < B))
            bufs, st = Bufs(eng, outs), _status()
            rc, err = _dev_call(eng, bufs, good, status=st)
            assert rc == 0, err
            _assert_only(bufs, truth, good, ("after", tag))
            assert st.tolist() == [OK, serial, -1, -1], (tag, st.tolist())
            serial += 1
        assert eng.list_errors() == (0, None)
        # two refusals counted together, the first one recorded
        bufs = Bufs(eng, outs)
        _dev_call(eng, bufs, [1, 1])
        _dev_call(eng, bufs, [B])
        n, first = eng.list_errors()
        assert n == 2 and first["code"] == TWICE and first["call"] == serial, (n, first)
        _assert_clean(bufs, "two refusals")
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. host refusals
def test_host_refusals_enqueue_nothing(def10, atk10):
    eng, B = def10, def10.B
    bufs = Bufs(eng, ("def", "def_code"))
    lib, h, s = _lib.lib, eng._h, eng._stream()

    def refused(rc, word, name):
        err = lib.td_last_error().decode()
        assert rc < 0 and err.startswith(name + ":") and word in err, (rc, err, word)
        _assert_clean(bufs, word)

    two = _ids32([1, 2])
    for name, call in (
            ("td_action_mask_boards", lambda io, ids, n: lib.td_action_mask_boards(h, io, ids, n, s)),
            ("td_action_mask_boards_dev", lambda io, ids, n: lib.td_action_mask_boards_dev(h, io, ids, n, None, None, s))):
        dev = name.endswith("_dev")
        ids = _dev(two) if dev else two
        p = ids.data_ptr() if dev else ids.ctypes.data
        refused(call(bufs.io(), p, B + 1), "outside [0, %d]" % B, name)  # n / cap > B
        refused(call(bufs.io(), None, 2), "NULL", name)  # NULL boards with n > 0
        refused(call(_lib.TdMaskIO(atk_mask=bufs.t["def"].data_ptr()), p, 2), "attacker", name)  # wrong side
        refused(call(_lib.TdMaskIO(def_mask=bufs.t["def"].data_ptr(), def_pitch=600), p, 2), "pitch", name)
        refused(call(_lib.TdMaskIO(), p, 2), "no output wanted", name)
        refused(call(_lib.TdMaskIO(def_mask=bufs.t["def"].data_ptr(), size=ctypes.sizeof(_lib.TdMaskIO) - 8), p, 2),
                "size", name)
        assert call(bufs.io(), p, 0) == 0  # an empty list: nothing launched
        assert call(bufs.io(), None, 0) == 0
        _assert_clean(bufs, "n = 0")
    # the contents of a host list are the host's to refuse
    rc, err = _host_call(eng, bufs, [3, B, 4])
    assert rc < 0 and err.startswith("td_action_mask_boards: entry 1: board %d outside" % B), err
    rc, err = _host_call(eng, bufs, [3, -1])
    assert rc < 0 and "entry 1: board -1 outside" in err, err
    rc, err = _host_call(eng, bufs, [3, 4, 3])
    assert rc < 0 and err.startswith("td_action_mask_boards: entry 2: board 3 is named twice"), err
    rc = lib.td_action_mask_boards(h, bufs.io(), two.ctypes.data, -1, s)
    assert rc < 0 and b"n = -1 outside" in lib.td_last_error()
    _assert_clean(bufs, "bad ids")
    # (and the scratch of the id check is clean again: the same boards are accepted now)
    truth = _full(eng, Bufs(eng, ("def", "def_code")))
    rc, err = _host_call(eng, bufs, [3, 4])
    assert rc == 0, err
    _assert_only(bufs, truth, [3, 4], "after the refusals")
    # TD-atk has no defender side
    ab = Bufs(atk10, ("atk",))
    rc = lib.td_action_mask_boards(atk10._h, _lib.TdMaskIO(def_code=ab.t["atk"].data_ptr()), two.ctypes.data, 2,
                                   atk10._stream())
    assert rc < 0 and b"td_action_mask_boards: TD-atk has no defender side" in lib.td_last_error()
    _assert_clean(ab, "atk")
    # the engine: host ids are not for the _dev form
    with pytest.raises(ValueError):
        eng.action_mask_boards_dev([1, 2])
    with pytest.raises(ValueError):
        eng.action_mask_boards_dev(torch.tensor([1, 2]))
    with pytest.raises(_lib.TDError):
        eng.action_mask_boards([1, 1])


# ------------------------------------------------------------------ 5. where the step's list forms refuse
def test_frame_skip_and_np_opponent_are_accepted():
    """Frame skip 3, and random_agent=False with auto-reset: both mask calls are accepted and
    equal the full call; td_step_boards and td_step_boards_dev refuse there."""
    cfg, hp = M.config(M.RICH), M.hyper(max_episode_steps=30)
    skip = _engine(10, 12, "def", False, cfg, hp, frame_skip=3)
    npa = _engine(10, 12, "def", False, cfg, hp, random_agent=False)
    try:
        for eng in (skip, npa):
            _random_steps(eng, 25, 3)  # (episodes of 30 steps: with frame skip across an episode end)
            noop = torch.full((eng.B,), 600, dtype=torch.int64)
            with pytest.raises(_lib.TDError):
                eng.step_boards([1, 2], def_act=noop)
            with pytest.raises(_lib.TDError):
                eng.step_boards_dev(_dev([1, 2]), def_act=noop)
            outs = ("def", "def_code")
            truth = _full(eng, Bufs(eng, outs))
            ids = [7, 0, 11, 4, 5]
            bufs = Bufs(eng, outs)
            rc, err = _host_call(eng, bufs, ids)
            assert rc == 0, err
            _assert_only(bufs, truth, ids, "host")
            bufs = Bufs(eng, outs)
            rc, err = _dev_call(eng, bufs, ids)
            assert rc == 0, err
            _assert_only(bufs, truth, ids, "dev")
            assert eng.list_errors() == (0, None)
    finally:
        skip.close()
        npa.close()


# ------------------------------------------------------------------ 6. the engine's methods
def test_engine_methods_write_the_engines_own_buffers(def10):
    eng = def10
    want = {k: v.clone() for k, v in eng.action_mask(code=True).items()}
    assert eng.action_mask_boards_kernel_name() == "td_mask_list_kernel<10>"
    for t in eng._mask_buf.values():
        t.fill_(SENT)
    ids = [5, 36, 0, 18]
    rest = [b for b in range(eng.B) if b not in ids]
    m = eng.action_mask_boards(ids, code=True)
    assert set(m) == {"def", "def_code"} and tuple(m["def"].shape) == (eng.B, 601)
    for k in m:
        assert m[k].data_ptr() == eng._mask_buf[k].data_ptr()
        assert torch.equal(m[k][ids], want[k][ids]) and bool((m[k][rest] == SENT).all()), k
    more = [1, 2]
    m = eng.action_mask_boards_dev(_dev(more))
    assert set(m) == {"def"}
    assert torch.equal(m["def"][ids + more], want["def"][ids + more])
    assert bool((eng._mask_buf["def_code"][more] == SENT).all())  # code not asked for: not written
    assert eng.action_mask_boards([])["def"].data_ptr() == eng._mask_buf["def"].data_ptr()
    assert eng.list_errors() == (0, None)


# ------------------------------------------------------------------ 7. TDVecEnv's partial refresh
class _Counter(object):
    """Counts the calls of some functions of _lib.lib while it is installed."""

    def __init__(self, names):
        self.n = dict.fromkeys(names, 0)
        self._real = {k: getattr(_lib.lib, k) for k in names}

    def __enter__(self):
        for k, fn in self._real.items():
            setattr(_lib.lib, k, self._wrap(k, fn))
        return self

    def _wrap(self, k, fn):
        def call(*a):
            self.n[k] += 1
            return fn(*a)
        return call

    def __exit__(self, *exc):
        for k, fn in self._real.items():
            setattr(_lib.lib, k, fn)


def _raw_truth(eng):
    """A full td_action_mask through the raw C call into separate buffers (engine.action_mask()
    would make the engine's own buffers current)."""
    t = _full(eng, Bufs(eng, ("def", "atk")))
    h = t.host()
    A = 6 * eng.L * eng.L + 1
    return t.rows("def", h["def"])[:, :A], t.rows("atk", h["atk"]).reshape(eng.B, 3, 5)


def test_vec_env_masks_always_equal_a_full_recompute():
    """B = 32 TD-2p, action_mask=True: a scripted sequence of 30 operations -- step, the four
    search calls with seeded lists, a config change of a tower price, a reset of some boards and a
    step through the engine behind the env's back, a device-refused fork_dev.  After every one
    the masks the env exposes equal a full recompute; and each search method took the partial
    call at least once (a sequence that always fell back would pass the comparison too)."""
    B, L = 32, 10
    env = E.TDVecEnv(L, B, "2p", seed=900, action_mask=True)
    eng = env.engine
    rng = np.random.RandomState(12)
    script = ["step", "step", "fork", "step_boards", "fork_dev", "step_boards_dev", "step_boards", "step",
              "step_boards_dev", "config", "step_boards", "fork", "fork", "engine_reset", "fork_dev", "step",
              "fork_dev", "refused_fork_dev", "step_boards_dev", "engine_step_boards", "step_boards", "fork",
              "step", "step_boards", "step_boards_dev", "config", "fork_dev", "step_boards_dev", "fork", "step_boards"]
    assert len(script) == 30
    partial = {}
    names = ("td_action_mask", "td_action_mask_boards", "td_action_mask_boards_dev")
    try:
        env.reset()
        assert eng.action_mask_boards_kernel_name() == "td_mask_list_kernel<10>"

        def acts():
            d = torch.from_numpy(rng.randint(0, 6 * L * L + 1, size=B).astype(np.int64)).to(DEV)
            a = torch.from_numpy(rng.randint(0, 5, size=(B, 3, 8)).astype(np.int64)).to(DEV)
            return {"Defender": d, "Attacker": a}

        def lists():
            p = rng.permutation(B)
            k = int(rng.randint(1, B // 2))
            return p[:k].tolist(), p[k:2 * k].tolist()

        for t, op in enumerate(script):
            src, dst = lists()
            with _Counter(names) as c:
                if op == "step":
                    env.step(acts())
                elif op == "step_boards":
                    env.step_boards(dst, acts())
                elif op == "step_boards_dev":
                    env.step_boards_dev(_dev(dst), acts())
                elif op == "fork":
                    env.fork(src, dst)
                elif op == "fork_dev":
                    env.fork_dev(_dev(src), _dev(dst), count=torch.tensor([len(dst)], dtype=torch.int32, device=DEV))
                elif op == "refused_fork_dev":
                    env.fork_dev(_dev(src + [src[0]]), _dev(dst + [dst[0]]))  # a destination twice
                elif op == "config":  # a tower price through the engine: every mask is void
                    cfg = copy.deepcopy(P.config)
                    cfg.tower_cost = [[1 + t % 3, 10], [17, 17], [23, 23], [2 + t % 5, 12]]
                    eng.set_config(cfg)
                    env.step_boards(dst, acts())
                elif op == "engine_reset":  # behind the env's back
                    m = np.zeros(B, dtype=np.uint8)
                    m[src] = 1
                    eng.reset(m)
                    env.fork(src[:1], dst[:1])
                elif op == "engine_step_boards":  # behind the env's back, then a search call
                    a = acts()
                    eng.step_boards(src, def_act=a["Defender"], atk_act=a["Attacker"])
                    env.step_boards(dst, acts())
            took = c.n["td_action_mask_boards"] + c.n["td_action_mask_boards_dev"]
            assert took + c.n["td_action_mask"] == 1, (t, op, c.n)  # one mask call per operation
            if op in ("config", "engine_reset", "engine_step_boards", "step"):
                assert took == 0, (t, op, c.n)  # the other rows were not known to be current
            elif took:
                partial[op] = partial.get(op, 0) + 1
                assert c.n["td_action_mask_boards_dev" if op.endswith("_dev") else "td_action_mask_boards"] == 1, (t, op)
            got = {k: v.cpu().numpy() for k, v in env._masks.items()}
            wd, wa = _raw_truth(eng)
            assert np.array_equal(got["def"], wd), (t, op, np.flatnonzero((got["def"] != wd).any(axis=1)))
            assert np.array_equal(got["atk"], wa), (t, op, np.flatnonzero((got["atk"] != wa).any(axis=(1, 2))))
        for op in ("step_boards", "step_boards_dev", "fork", "fork_dev", "refused_fork_dev"):
            assert partial.get(op, 0) >= 1, (op, partial)
        n, first = eng.list_errors()
        assert n == 2 and first["code"] == TWICE, (n, first)  # the refused fork and its refused mask list
    finally:
        env.close()
