"""Device board lists longer than one block of the check kernel (td_step_boards_dev,
td_copy_boards_dev, td_action_mask_boards_dev at 2,100 boards).

csrc/td_list_check.hip judges a list with one thread per entry in blocks of 256.  With more than
256 entries the check is several blocks that meet only through atomics: the ticket counter that
lets the last block build the verdict, the marks two conflicting entries of different blocks
find each other by, the defect key as a minimum over blocks.  The consumers behind it place
their work with a count the host never sees.  tests/test_gpu_board_lists_dev.py pins all of this
inside one block; this file pins it at 2,100 boards = 9 check blocks, the last one partial and
shorter than a wave (tests/listcases.py has the lists and says which block lies where;
tests/test_list_cases_host.py proves the table and its reference without a GPU).

The verdict's judge is tests/listref.py, a plain restatement of include/tdstep.h.  The judge of
everything else is the twin of tests/test_gpu_board_lists_dev.py, whose helpers are imported
unchanged: engine A takes the device-list calls, engine B the host-list calls with the same ids,
and all 2,100 boards are compared byte for byte -- the output tensors on the device after every
call, the exported state (it holds the opponent's stream), flags, episode records and count with
them, and everything _snap() holds, both RNG streams included, at the end of every test (a stream
that has diverged stays diverged).  The one tolerance is _sum_tolerance, as there.  No test
provokes a fault: every bad list is one the check kernel is specified to refuse, and a refused
consumer reads no id."""
import numpy as np
import pytest
import torch

import listcases as C

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

import test_gpu_board_lists_dev as T  # noqa: E402  (its helpers: the twin, its snapshot, its tolerance)

B = C.B
OK, TWICE = C.OK, C.TWICE
SENT = 0xA5  # the mask buffers' sentinel, as tests/test_gpu_action_mask_boards.py
_dev, _status, _draw = T._dev, T._status, T._draw


# ------------------------------------------------------------------ helpers
def _engine(**kw):
    kw.setdefault("hp", T._short())
    kw.setdefault("autoreset", True)
    return T._engine(10, n=B, **kw)


def _outs(eng):
    """Clones of every output tensor, on the device."""
    return {n: getattr(eng, n).view(torch.uint8).clone() for n in T.OUTPUTS if getattr(eng, n) is not None}


def _assert_outs(eng, want, tag):
    """eng's output tensors against clones (or against another engine's), on the device."""
    want = want if isinstance(want, dict) else {n: getattr(want, n).view(torch.uint8) for n in T.OUTPUTS
                                                 if getattr(want, n) is not None}
    for n, w in want.items():
        assert torch.equal(getattr(eng, n).view(torch.uint8), w), (tag, n)


def _rest(eng):
    """What _snap holds beside the outputs and the per-board streams: the exported state, the
    flags, the episode records, their count and sum."""
    torch.cuda.synchronize()
    s = {}
    for k, v in eng.export_state().items():
        s["state." + k] = np.ascontiguousarray(v).tobytes()
    s["flags"] = eng.flags().tobytes()
    for k, t in zip(("ret", "len", "win"), eng.episode_records()):
        s["rec." + k] = t.cpu().numpy().tobytes()
    stats = eng.episode_stats().cpu().numpy()
    s["stats.n"] = stats[:1].tobytes()
    s[T.SUM] = float(stats[1])
    return s


def _assert_twins(a, b, tag):
    _assert_outs(a, b, tag)
    T._assert_same(_rest(a), _rest(b), tag)


def _count(row):
    return None if row.count is None else _dev([row.count])


class Masks(object):
    """The engine's own mask and code buffers under a sentinel, and the full call's bytes."""

    def __init__(self, eng):
        self.eng = eng
        eng.action_mask(code=True)
        torch.cuda.synchronize()
        self.truth = {k: eng._mask_buf[k].clone() for k in ("def", "def_code")}
        self.fill()

    def fill(self):
        for k in self.truth:
            self.eng._mask_buf[k].fill_(SENT)

    def assert_only(self, named, tag):
        """Every row is the sentinel, but the named rows: those are the full call's."""
        torch.cuda.synchronize()
        idx = torch.as_tensor(np.asarray(named, dtype=np.int64), device=T.DEV)
        for k, t in self.truth.items():
            want = torch.full_like(t, SENT)
            want[idx] = t[idx]
            got = self.eng._mask_buf[k]
            assert torch.equal(got, want), (tag, k, torch.nonzero((got != want).any(dim=1)).flatten()[:8].tolist())


def _rows(kind):
    return [r for r in C.table() if r.kind == kind]


# ------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("kind", ["step", "copy+", "copy-", "mask"])
def test_table_rows(kind):
    """Every row of tests/listcases.py of one kind, in the table's order, on one pair of twins.
    A refused row: the status is the code tests/listref.py gives with one of the (entry, board)
    pairs it allows, td_list_errors reports that record once, no byte of any output, of the state,
    the flags or the records changed, and the valid list of the same boards then works on A as
    its host form does on B.  An accepted row: A's
    device call against B's host call with ids[:n].  The streams: the closing _snap."""
    rows = _rows(kind)
    copy, mask = kind.startswith("copy"), kind == "mask"
    a, b = _engine(), _engine()
    try:
        rng = np.random.RandomState(31)
        for _ in range(6 if mask else 3):
            acts = _draw(rng, a)
            a.step(**acts)
            b.step(**acts)
        ma, mb = (Masks(a), Masks(b)) if mask else (None, None)
        serial = refused = 0

        def call(eng_dev, src, dst, count, st, acts):
            if kind == "step":
                eng_dev.step_boards_dev(_dev(dst), count=count, status=st, **acts)
            elif mask:
                eng_dev.action_mask_boards_dev(_dev(dst), count=count, status=st, code=True)
            else:
                eng_dev.copy_boards_dev(_dev(src), _dev(dst), count=count, write_obs=kind == "copy+", status=st)

        def host(src, dst, acts):
            if kind == "step":
                b.step_boards(dst, **acts)
            elif mask:
                b.action_mask_boards(dst, code=True)
            elif len(dst):
                b.copy_boards(src, dst, write_obs=kind == "copy+")

        for row in rows:
            code, allowed = C.expect(row)
            n = C.used(row)
            acts = _draw(rng, a)
            st = _status()
            if code == OK:
                call(a, row.src, row.dst, _count(row), st, acts)
                host(None if row.src is None else row.src[:n], row.dst[:n], acts)
                torch.cuda.synchronize()
                assert st.tolist() == [OK, serial, -1, -1], (row.name, st.tolist())
                serial += 1
                named = row.dst[:n]
            else:
                before = _outs(a)
                rest = _rest(a)
                call(a, row.src, row.dst, _count(row), st, acts)
                torch.cuda.synchronize()
                got = st.tolist()
                assert got[:2] == [code, serial] and (got[2], got[3]) in allowed, (row.name, got, code, sorted(allowed)[:6])
                nerr, first = a.list_errors()
                assert nerr == 1 and first == dict(code=code, call=serial, entry=got[2], board=got[3]), (row.name, nerr, first)
                assert a.list_errors() == (0, None), row.name
                _assert_outs(a, before, ("refused", row.name))
                if mask:
                    ma.assert_only([], ("refused", row.name))
                T._assert_same(_rest(a), rest, ("refused", row.name))
                serial += 1
                refused += 1
                # the valid list of the same boards, right behind the refusal
                fs, fd = row.follow
                st = _status()
                call(a, fs, fd, None, st, acts)
                host(fs, fd, acts)
                torch.cuda.synchronize()
                assert st.tolist() == [OK, serial, -1, -1], (row.name, st.tolist())
                serial += 1
                named = fd
            _assert_twins(a, b, row.name)
            if mask:
                ma.assert_only(named, row.name)
                mb.assert_only(named, (row.name, "host list"))
                ma.fill()
                mb.fill()
            if copy:  # (the boards move on between two copies)
                acts = _draw(rng, a)
                a.step(**acts)
                b.step(**acts)
        assert refused >= 8 and serial == len(rows) + refused
        assert a.list_errors() == (0, None)
        T._assert_same(T._snap(a), T._snap(b), "the end")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 2. every board, shuffled
def test_all_boards_shuffled_equal_plain_steps():
    """A list of all 2,100 boards in a fresh shuffled order per call, 20 calls (episodes of 16
    steps: every board ends one through the list form's auto-reset), against an engine that calls
    plain step(), which the rest of the suite pins to the oracle.  The opponent's stream is
    compared in CPython's form (_snap's "py"): the raw words of the exported state depend on how
    far a kernel has carried its lazy twist, and step() runs another kernel than the list."""
    def canon(s):
        return {k: v for k, v in s.items() if k != "state.opp_mt"}

    a, c = _engine(), _engine()
    try:
        rng = np.random.RandomState(58)
        for t in range(20):
            acts = _draw(rng, a)
            ids = rng.permutation(B).astype(np.int32)
            st = _status()
            if t % 2:
                a.step_boards_dev(_dev(ids), count=_dev([B]), status=st, **acts)
            else:
                a.step_boards_dev(_dev(ids), status=st, **acts)
            c.step(**acts)
            torch.cuda.synchronize()
            assert st.tolist() == [OK, t, -1, -1]
            _assert_outs(a, c, t)
            if t % 5 == 4:
                T._assert_same(canon(_rest(a)), canon(_rest(c)), t)
        assert (a.episode_records()[1].cpu().numpy() > 0).all()
        assert a.list_errors() == (0, None)
        T._assert_same(canon(T._snap(a)), canon(T._snap(c)), "the end")
    finally:
        a.close()
        c.close()


# ------------------------------------------------------------------ 3. back to back, the grid changing
CAPS = (90, 2100, 700, 257)  # 1, 9, 3 and 2 check blocks


def _script(rng, calls=40):
    """(kind, src, dst, count, refused): call t has cap CAPS[t % 4] and is a copy if t % 3 == 2,
    else a step.  A copy of cap 2,100 goes through a count of 1,000 with poison behind it (no
    valid copy names every board as a destination).  Call 13, a step list of 2,100: a board twice,
    at entries 10 and 1,300 (blocks 0 and 5).  Call 26, a copy of 700: entry 650's destination
    (block 2) is entry 20's source (block 0)."""
    out = []
    for t in range(calls):
        cap = CAPS[t % 4]
        perm = rng.permutation(B).astype(np.int32).tolist()
        if t % 3 != 2:
            ids = perm[:cap]
            if t == 13:
                assert cap == B
                ids[1300] = ids[10]
            out.append(("step", None, ids, None, t == 13))
        else:
            n = min(cap, 1000)
            src, dst, count = perm[:n], perm[n:2 * n], None
            if t == 26:
                assert cap == 700
                dst[650] = src[20]
            if n < cap:
                count = n
                src = src + [-7] * (cap - n)
                dst = dst + [dst[i % n] for i in range(cap - n)]
            out.append(("copy", src, dst, count, t == 26))
    assert [x[4] for x in out].count(True) == 2
    return out


def _run_script(eng, script, acts, device_lists, sync):
    for (kind, src, dst, count, bad), act in zip(script, acts):
        n = len(dst) if count is None else count
        cnt = None if count is None else _dev([count])
        if kind == "step":
            if device_lists:
                eng.step_boards_dev(_dev(dst), count=cnt, **act)
            elif not bad:
                eng.step_boards(dst[:n], **act)
        else:
            if device_lists:
                eng.copy_boards_dev(_dev(src), _dev(dst), count=cnt, write_obs=True)
            elif not bad:
                eng.copy_boards(src[:n], dst[:n], write_obs=True)
        if sync:
            torch.cuda.synchronize()


def test_forty_calls_back_to_back_with_a_changing_grid():
    """No synchronisation between forty calls whose checks have 1, 9, 3, 2, 1, ... blocks: the
    last block of one check leaves key and ticket counter to a check of another grid in stream
    order alone.  Against the same script with a sync after every call, and with host lists."""
    engines = [_engine() for _ in range(3)]
    try:
        rng = np.random.RandomState(79)
        script = _script(rng)
        acts = [_draw(rng, engines[0]) for _ in script]
        torch.cuda.synchronize()
        _run_script(engines[0], script, acts, True, False)
        _run_script(engines[1], script, acts, True, True)
        _run_script(engines[2], script, acts, False, True)
        snaps = [T._snap(e) for e in engines]
        T._assert_same(snaps[0], snaps[1], "no sync vs sync")
        T._assert_same(snaps[0], snaps[2], "device lists vs host lists")
        for e in engines[:2]:
            n, first = e.list_errors()
            assert n == 2 and first["call"] == 13 and first["code"] == TWICE and first["entry"] in (10, 1300), (n, first)
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------ 4. the retained buffer
def test_retained_buffer_equals_a_twin_that_writes_every_byte():
    """The plan of test_retained_buffer_always_equals_a_twin_that_writes_every_byte of
    tests/test_gpu_board_lists_dev.py at 2,100 boards, lists of 300 to 1,000 ids."""
    a = _engine(sentinel=False, retain_obs=True)
    b = _engine(sentinel=False, retain_obs=False)
    try:
        assert a.retain_obs and not b.retain_obs
        rng = np.random.RandomState(9)
        plan = ["step", "step", "list", "list", "step", "copy+", "list", "step", "step", "copy-", "list", "step", "copy+",
                "copy-", "step", "list", "copy+", "step", "step", "list"]
        for t, what in enumerate(plan):
            acts = _draw(rng, a)
            perm = rng.permutation(B).astype(np.int32)
            k = int(rng.randint(300, 1001))
            if what == "step":
                a.step(**acts)
                b.step(**acts)
            elif what == "list":
                a.step_boards_dev(_dev(perm[:k]), **acts)
                b.step_boards(perm[:k], **acts)
            else:
                a.copy_boards_dev(_dev(perm[:k]), _dev(perm[k:2 * k]), write_obs=what == "copy+")
                b.copy_boards(perm[:k], perm[k:2 * k], write_obs=what == "copy+")
            torch.cuda.synchronize()
            assert torch.equal(a.obs, b.obs), (t, what)
        assert a.list_errors() == (0, None)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 5. the full fan-out
@pytest.mark.parametrize("write_obs", [True, False])
def test_full_fan_out_then_three_steps(write_obs):
    """One root, 2,099 children in one td_copy_boards_dev (every wave of the check marks the one
    source once), then three steps of every board through shuffled device lists."""
    a, b = _engine(), _engine()
    try:
        rng = np.random.RandomState(14)
        for _ in range(5):
            acts = _draw(rng, a)
            a.step(**acts)
            b.step(**acts)
        root = 1234
        kids = [x for x in rng.permutation(B).tolist() if x != root]
        st = _status()
        a.copy_boards_dev(_dev([root] * len(kids)), _dev(kids), write_obs=write_obs, status=st)
        b.copy_boards([root] * len(kids), kids, write_obs=write_obs)
        torch.cuda.synchronize()
        assert st.tolist() == [OK, 0, -1, -1]
        _assert_twins(a, b, "copy")
        for t in range(3):
            acts = _draw(rng, a)
            ids = rng.permutation(B).astype(np.int32)
            a.step_boards_dev(_dev(ids), status=st, **acts)
            b.step_boards(ids, **acts)
            torch.cuda.synchronize()
            assert st.tolist() == [OK, 1 + t, -1, -1]
            _assert_twins(a, b, ("step", t))
        assert a.list_errors() == (0, None)
        T._assert_same(T._snap(a), T._snap(b), "the end")
    finally:
        a.close()
        b.close()
