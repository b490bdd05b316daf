"""The call surface on a caller's stream, pinned to its default-stream twin.

Every other GPU test drives the library on torch's default stream, the legacy NULL stream, where
the step stream and the NULL stream are one queue.  Here engine T, the twin, is driven that way
(the rest of the suite pins it to the oracle) and engine A gets the same seeds, config and calls
inside ``with torch.cuda.stream(S)``, S a non-blocking stream of its own that lags behind the
host: in front of every group of calls a spin is enqueued on S (streamutil.lag), the group is
issued without a synchronisation of the test's own, and then everything A holds is compared with
T at the same point (streamutil.snapshot / same).  A kernel, copy, memset or event that lands on
another stream than S, or a NULL-stream runtime call that a launch on S overtakes, runs early and
leaves a difference.  Everything is compared byte for byte but two things: the atomic sum of
returns (streamutil.sum_tolerance) and, while refills stage layouts ahead on the side streams, how
far ahead a board's layout stream has been drawn, which depends on timing by design: there it must
be the twin's stream at another lead (streamutil.same).  With a refill interval of 0, with
random_agent=False and without auto-reset the layout streams are compared byte for byte too.

Vacuity: right after the last call of a group the test asks whether S still has work queued
(streamutil.ran_ahead).  Of the groups that hold only asynchronous calls at least half must say
yes, or the test fails as vacuous; each test's docstring carries the share observed on an MI355X.
This shows that the host ran ahead of the stream.  It does not show which hardware queue S got:
that a handle's two side streams, S and the NULL stream share the process's four hardware queues
is assumed from the runtime's setting, not observed.

Left out: one round of the device lists' mark epochs (td_list_check.h kListEpochs = 2^30 - 1
list calls); hipGraph capture, moving a handle between streams, more than two handles, multi-GPU.
No test provokes a fault: every refused list is one the check kernel is specified to catch.
"""
import contextlib
import copy
import ctypes
import random

import numpy as np
import pytest
import torch

import handmaps as H
import maskutil as M
import steputil
import streamutil as U

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import envs as E  # noqa: E402
from gym_TD import params as P  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402
from oracle import policies  # noqa: E402
from oracle import td_oracle as O  # noqa: E402

DEV = torch.device("cuda", 0)
EP = 24          # max_episode_steps: 120 steps end every board's episode about five times
GROUP = 8        # calls per group
RANGE, TWICE = 2, 3  # td_list_code


# ------------------------------------------------------------------ the pattern
def _hp(multi=False):
    return M.hyper(multi, max_episode_steps=EP)


def _acts(eng, steps, seed=5):
    """``steps`` steps of uniform random actions for every board, on the device already: a step
    takes row k as it is, no copy from the host (which would wait for the stream)."""
    rng = np.random.RandomState(seed)
    L, n, d, a = eng.L, eng.B, None, None
    if eng.mode != "atk":
        d = ((rng.random_sample((steps, n, 6, L, L)) < 0.02).astype(np.int64) if eng.multi
             else rng.randint(0, 6 * L * L + 1, size=(steps, n)).astype(np.int64))
        d = torch.from_numpy(d).to(DEV)
    if eng.mode != "def":
        a = torch.from_numpy(rng.randint(0, 5, size=(steps, n, 3, 8)).astype(np.int64)).to(DEV)
    return d, a


def _act(c, k):
    d, a = c["acts"]
    return dict(def_act=None if d is None else d[k], atk_act=None if a is None else a[k])


def _mk(L=10, B=33, mode="def", multi=False, steps=120, refill=None, seed0=1700, **kw):
    """make(c): an engine of short episodes, reset, with its actions and a per-board count of
    ``done`` on the device in the run's record ``c``."""
    def make(c):
        seeds = seed0 + np.arange(B)
        kw2 = dict(hp=_hp(multi))
        kw2.update(kw)
        eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, **kw2)
        eng.reset_all()
        if refill is not None:
            eng.set_refill_interval(refill)
        c["acts"] = _acts(eng, steps)
        c["dones"] = torch.zeros(B, dtype=torch.int32, device=DEV)
        c["refill"] = refill  # (None: the library's own interval)
        return eng
    return make


class _Run(object):
    """One engine and the generator that drives it.  The generator yields "lag" (a spin goes in
    front of what follows; nothing on the twin), "call" (one call was issued: where two runs
    alternate) or ``(extras, only_async)`` at a group's end: the snapshot is taken there and, with
    ``want`` (the twin's snapshots), compared.  Everything runs inside ``with
    torch.cuda.stream(stream)`` (None: the default stream, the twin); ``busy``: the spin goes on
    the default stream too; ``outside``: the engine is made on the default stream."""

    def __init__(self, make, drive, stream=None, want=None, tag="", busy=False, outside=False):
        self.S, self.want, self.tag, self.busy = stream, want, tag, busy
        self.c, self.snaps, self.ahead, self.async_groups, self.over, self.pending = {}, [], 0, 0, False, None
        with contextlib.nullcontext() if outside else self._ctx():
            self.eng = make(self.c)
        torch.cuda.synchronize()
        self.gen = drive(self.eng, self.c)

    def _ctx(self):
        return torch.cuda.stream(self.S) if self.S is not None else contextlib.nullcontext()

    def advance(self):
        """One item of the generator.  True at a group's end: ran_ahead has been asked, and
        settle() takes the snapshot (two runs that alternate ask both before either waits)."""
        with self._ctx():
            try:
                item = next(self.gen)
            except StopIteration:
                self.over = True
                return False
            except BaseException:
                self.eng.close()
                raise
            if isinstance(item, str):
                if item == "lag" and self.S is not None:
                    if self.busy:
                        U.lag(torch.cuda.default_stream(DEV))
                    U.lag(self.S)
                return False
            extras, only_async = item
            if self.S is not None and only_async:
                self.async_groups += 1
                self.ahead += bool(U.ran_ahead(self.S))
            self.pending = extras
            return True

    def settle(self):
        with self._ctx():
            try:
                snap = U.snapshot(self.eng, self.pending)
                g = len(self.snaps)
                if self.want is not None:
                    assert g < len(self.want), (self.tag, "more groups than the twin")
                    e = self.eng  # (layouts staged ahead on the side streams: streamutil.same)
                    lead = e.autoreset and e.random_agent and self.c.get("refill") != 0
                    U.same(snap, self.want[g], "%s, group %d" % (self.tag, g), np_lead=lead)
            except BaseException:
                self.eng.close()
                raise
            self.snaps.append(snap)

    def run(self):
        while not self.over:
            if self.advance():
                self.settle()
        return self

    def finish(self):
        with self._ctx():
            torch.cuda.synchronize()
            e = self.eng
            try:
                assert (e.flags() == 0).all(), (self.tag, e.flags().tolist())
                assert e.guard_timeouts() == 0, self.tag
                assert e.list_errors() == self.c.get("list_errors", (0, None)), self.tag
                if self.want is not None:
                    assert len(self.snaps) == len(self.want), self.tag
                if self.S is not None:
                    print("%s: ran_ahead held for %d of %d asynchronous groups" % (self.tag, self.ahead, self.async_groups))
                    assert self.async_groups > 0, self.tag
                    assert 2 * self.ahead >= self.async_groups, \
                        "%s is vacuous: the host ran ahead of the stream in %d of %d groups" % (self.tag, self.ahead,
                                                                                               self.async_groups)
            finally:
                e.close()
        return self


def _twins(make, drive, tag, stream=None, **kw):
    """The twin on the default stream, then A on ``stream`` (None: a new torch.cuda.Stream())
    against the twin's snapshots.  Returns both runs' records."""
    t = _Run(make, drive, tag=tag + " twin").run().finish()
    S = torch.cuda.Stream(DEV) if stream is None else stream
    assert S.cuda_stream != 0
    a = _Run(make, drive, stream=S, want=t.snaps, tag=tag, **kw).run().finish()
    return t.c, a.c


def _drive_rollout(steps, stats_every=0):
    """``steps`` steps in groups of GROUP.  stats_every: episode_stats(clear) and
    episode_records() inside the groups, every so many steps."""
    def drive(eng, c):
        c["counts"], c["sums"] = [], []
        extras = {}
        for k in range(steps):
            if k % GROUP == 0:
                yield "lag"
            eng.step(**_act(c, k))
            c["dones"] += eng.done
            if stats_every and (k + 1) % stats_every == 0:
                st = eng.episode_stats(clear=True)
                c["counts"].append(st[:1])
                c["sums"].append(st[1:])
                for name, t in zip(("ret", "len", "win"), eng.episode_records()):
                    extras["rec%d.%s" % (k, name)] = t
            if (k + 1) % GROUP == 0 or k + 1 == steps:
                if c["counts"]:
                    extras["counts"] = torch.cat(c["counts"]).reshape(1, -1)
                yield extras, True
                extras = {}
    return drive


def _episodes_per_board(c, eng_B, least):
    """Every board finished at least ``least`` episodes, by its count of ``done``."""
    dones = c["dones"].cpu().numpy()
    assert dones.shape == (eng_B,) and dones.min() >= least, dones.tolist()
    return int(dones.sum())


def _check_finished(t, a, B, least=4):
    """At least ``least`` finished episodes per board, from the count of ``done``, the records'
    lengths and the episode count."""
    for c in (t, a):
        total = _episodes_per_board(c, B, least)
        assert c["final"]["n"] == total, (c["final"]["n"], total)
        assert (c["final"]["len"] > 0).all() and (c["final"]["win"] >= 0).all()


def _drive_rollout_final(steps):
    """_drive_rollout, with the episode count and records read at the end."""
    inner = _drive_rollout(steps)

    def drive(eng, c):
        for item in inner(eng, c):
            yield item
        _, ln, win = eng.episode_records()
        c["final"] = dict(n=int(eng.episode_stats()[0].item()), len=ln.cpu().numpy(), win=win.cpu().numpy())
    return drive


# ------------------------------------------------------------------ 1-3: rollouts
@pytest.mark.parametrize("refill,dtype,kernel", [
    (4, torch.float32, "auto"), (0, torch.float32, "auto"), (4, torch.float16, "auto"), (0, torch.float16, "auto"),
    (4, torch.float32, "large"), (4, torch.float32, "small"), (4, torch.float32, "small2")])
def test_rollout_autoreset(refill, dtype, kernel):
    """120 steps of TD-def 10x10, 33 boards, auto-reset, retained observation: with a refill every
    4th step (both side streams, each anchored to S by ev_step) and with none (every layout from
    the ring guard on S), float32 and float16, and on each step kernel.  Every board finishes at
    least 4 episodes.  ran_ahead: 15 of 15 groups in every case."""
    make = _mk(refill=refill, obs_dtype=dtype, step_kernel=kernel)
    t, a = _twins(make, _drive_rollout_final(120), "rollout refill=%d %s %s" % (refill, dtype, kernel))
    _check_finished(t, a, 33)


def test_rollout_random_agent_false():
    """random_agent=False with auto-reset: the reset kernel behind every step on S
    (launch_autoreset), 120 steps, at least 4 episodes per board.  ran_ahead: 15 of 15 groups."""
    t, a = _twins(_mk(random_agent=False), _drive_rollout_final(120), "random_agent=False")
    _check_finished(t, a, 33)


def test_rollout_frame_skip():
    """Frame skip 3, 40 macro steps.  ran_ahead: 5 of 5 groups."""
    _twins(_mk(frame_skip=3), _drive_rollout(40), "frame skip 3")


# ------------------------------------------------------------------ 4: synchronous calls
def _second_config():
    cfg = copy.deepcopy(P.config)
    cfg.tower_cost = [[14, 14], [17, 17], [23, 23], [12, 12]]
    cfg.max_cost = 80
    return cfg


def _hand_records(n):
    recs = [H.record(H.MAPS[name][1], 10) for name in ("snake64", "border")]
    return np.stack([recs[i % len(recs)] for i in range(n)])


def _sync_calls(B):
    rng = np.random.RandomState(21)
    half = (rng.random_sample(B) < 0.5).astype(np.uint8)
    some = (rng.random_sample(B) < 0.5).astype(np.uint8)
    boards = rng.permutation(B)[:B // 3].astype(np.int32)

    def reseed(e):
        e.seed(np_seeds=5000 + np.arange(B), py_seeds=6000 + np.arange(B))

    def rng_states(e):
        e.set_np_state(2, np.random.RandomState(777).get_state())
        e.set_py_state(3, random.Random(778).getstate())

    return [("reset(mask)", lambda e: e.reset(half)),
            ("reset_layouts", lambda e: e.reset_layouts(_hand_records(len(boards)), boards)),
            ("opponent", lambda e: e.opponent("enemy", 1, some)),
            ("set_config", lambda e: e.set_config(_second_config(), _hp())),
            ("seed", reseed),
            ("set_np_state / set_py_state", rng_states),
            ("export_state / import_state", lambda e: e.import_state(e.export_state(1, 1), 0))]


def test_synchronous_calls_between_lagging_groups():
    """reset(mask), reset_layouts, opponent, set_config, seed, set_np_state / set_py_state and
    export_state / import_state, each called mid-run with a spin queued on S in front of it and
    six steps behind it in the same group, groups of eight steps alone in between: the NULL-stream
    copies and memsets of these calls against the launches on S, and on the side streams, that
    follow.  ran_ahead: 8 of 8 asynchronous groups."""
    calls = _sync_calls(33)

    def drive(eng, c):
        k = 0
        for name, call in [(None, None)] + calls:
            yield "lag"
            for _ in range(GROUP):
                eng.step(**_act(c, k))
                k += 1
            yield {}, True
            if call is not None:
                yield "lag"
                call(eng)
                for _ in range(6):
                    eng.step(**_act(c, k))
                    k += 1
                yield {}, False

    _twins(_mk(refill=4), drive, "synchronous calls")


def test_reset_layouts_two_chunks():
    """td_reset_layouts' loop over chunks of stage_cap = 4,096 boards: 4,200 boards at 10x10 reset
    whole from cycled hand layouts in one call behind a spin (two chunks, the second of 104
    boards), then one step; the exported layouts and the observations equal the twin's."""
    B = 4200
    recs, ids = _hand_records(B), np.arange(B, dtype=np.int32)
    got = []
    for S in (None, torch.cuda.Stream(DEV)):
        with torch.cuda.stream(S) if S is not None else contextlib.nullcontext():
            seeds = np.arange(B)
            eng = TDEngine(10, B, "def", False, 1, np_seeds=seeds, py_seeds=seeds, hp=_hp(), autoreset=True)
            try:
                act = torch.full((B,), 600, dtype=torch.int64, device=DEV)
                torch.cuda.synchronize()
                if S is not None:
                    U.lag(S)
                eng.reset_layouts(recs, ids)
                first = eng.obs.clone()
                eng.step(def_act=act)
                st = eng.export_state()
                got.append(dict(obs0=first.cpu().numpy().tobytes(), obs1=eng.obs.cpu().numpy().tobytes(),
                                cells=st["cells"].tobytes(), hdr=st["hdr"].tobytes()))
                assert (eng.flags() == 0).all()
            finally:
                eng.close()
    for k in got[0]:
        assert got[1][k] == got[0][k], k


# ------------------------------------------------------------------ 5: host board lists
def _drive_host_lists(groups=6):
    def drive(eng, c):
        rng = np.random.RandomState(11)
        B, k = eng.B, 0
        yield "lag"
        for _ in range(GROUP):
            eng.step(**_act(c, k))
            k += 1
        yield {}, True
        for _ in range(groups):
            yield "lag"
            for j in range(9):  # more than two rounds of the four pinned id slots
                if j % 2 == 0:
                    perm = rng.permutation(B)
                    if j == 2:  # one source, 16 destinations
                        src, dst = np.full(16, perm[0]), perm[1:17]
                    else:
                        n = rng.randint(1, B // 2)
                        src, dst = perm[:n], perm[n:2 * n]
                    src, dst = src.astype(np.int32), dst.astype(np.int32)
                    eng.copy_boards(src, dst)
                    src[:] = 0  # the caller's arrays are the caller's again on return
                    dst[:] = 0
                else:
                    ids = rng.permutation(B)[:rng.randint(1, B)].astype(np.int32)
                    eng.step_boards(ids, **_act(c, k))
                    k += 1
                    ids[:] = 0
            yield {}, False  # (the fifth call of a group waits for the first one's id upload)
    return drive


def test_host_board_lists():
    """Nine copy_boards / step_boards calls back to back behind one spin, six times: other ids in
    every call, a fan-out from one source to 16 destinations among them, and the caller's numpy
    arrays overwritten right after each call.  From the fifth call on, a call waits for the id
    upload four calls before it (upload_ids), so these groups are not asynchronous ones.
    ran_ahead: 1 of 1 asynchronous group (the eight steps in front)."""
    _twins(_mk(), _drive_host_lists(), "host board lists")


# ------------------------------------------------------------------ 6: device board lists
def _not_done(eng):
    """The boards that are not done, compacted to the front of a buffer of B ids, and their
    number, without the host looking (torch.nonzero would bring the count to the host)."""
    done = eng.done != 0
    ids = torch.argsort(done.to(torch.int8), stable=True).to(torch.int32)
    return ids, (~done).sum().to(torch.int32).reshape(1)


def _status(n):
    return torch.full((n, 4), -99, dtype=torch.int32, device=DEV)


def _no_twice_entry(st):
    """The status words for the comparison with the twin: of two entries that name one board the
    device may report either (whichever marks second), so that word is left out."""
    st = st.clone()
    st[:, 2] = torch.where(st[:, 0] == TWICE, torch.full_like(st[:, 2], -1), st[:, 2])
    return st


def test_device_board_lists_built_on_the_stream():
    """The ids are built by torch on S from the step's ``done`` and consumed by step_boards_dev,
    copy_boards_dev and action_mask_boards_dev in the same group; a list with an id out of range
    and one that names a board twice are in every group, their status words read in stream order.
    Then list_errors(clear=True), followed at once on S by one more refused list and an accepted
    one: the next list_errors() reports exactly that one refusal.  One round of the mark epochs
    is 2^30 - 1 list calls (td_list_check.h kListEpochs): not run.  ran_ahead: 4 of 4
    asynchronous groups."""
    B, n_groups = 33, 4

    def drive(eng, c):
        rng = np.random.RandomState(13)
        k = serial = 0
        for g in range(n_groups):
            perm = rng.permutation(B)
            src = torch.from_numpy(perm[:6].astype(np.int32)).to(DEV)
            dst = torch.from_numpy(perm[6:12].astype(np.int32)).to(DEV)
            bad_range = torch.from_numpy(np.array([1, 2, B + 5, 4], dtype=np.int32)).to(DEV)
            bad_twice = torch.from_numpy(np.array([3, 7, 9, 7], dtype=np.int32)).to(DEV)
            st = _status(5)
            torch.cuda.synchronize()
            yield "lag"
            eng.step(**_act(c, k))
            ids, count = _not_done(eng)
            eng.step_boards_dev(ids, count=count, status=st[0], **_act(c, k + 1))
            eng.copy_boards_dev(src, dst, status=st[1])
            masks = eng.action_mask_boards_dev(ids, count=count, status=st[2])
            eng.step_boards_dev(bad_range, status=st[3], **_act(c, k + 2))
            eng.copy_boards_dev(src[:4], bad_twice, status=st[4])
            k += 3
            yield dict(status=_no_twice_entry(st), ids_used=count.reshape(1, 1), mask=masks["def"].clone()), True
            want = [0, 0, 0, RANGE, TWICE]
            assert st[:, 0].tolist() == want, st.tolist()
            assert st[:, 1].tolist() == list(range(serial, serial + 5)), st.tolist()
            assert st[3].tolist()[2:] == [2, B + 5], st.tolist()
            assert st[4, 2].item() in (1, 3) and st[4, 3].item() == 7, st.tolist()
            first = dict(code=RANGE, call=serial + 3, entry=2, board=B + 5)
            serial += 5
            # the clear's NULL-stream memsets against the check kernel of the next call on S
            st2 = _status(2)
            torch.cuda.synchronize()
            yield "lag"
            assert eng.list_errors(clear=True) == (2, first)
            eng.copy_boards_dev(src[:4], bad_twice, status=st2[0])
            eng.step_boards_dev(ids, count=count, status=st2[1], **_act(c, k))
            k += 1
            yield dict(status=_no_twice_entry(st2)), False
            n, rec = eng.list_errors(clear=True)
            assert n == 1 and rec["entry"] in (1, 3), (n, rec)
            assert dict(rec, entry=3) == dict(code=TWICE, call=serial, entry=3, board=7), rec
            serial += 2

    _twins(_mk(), drive, "device board lists")


# ------------------------------------------------------------------ 7: masks
@pytest.mark.parametrize("L,B,mode,multi", [(10, 33, "def", False), (20, 9, "2p", True)])
def test_masks_behind_steps(L, B, mode, multi):
    """action_mask(code=True) and action_mask_boards after six steps in the same group, compared
    as bytes with the twin's.  ran_ahead: 5 of 5 groups in both cases."""
    def drive(eng, c):
        rng = np.random.RandomState(17)
        for g in range(5):
            yield "lag"
            for k in range(6 * g, 6 * g + 6):
                eng.step(**_act(c, k))
            extras = {"full." + n: t.clone() for n, t in eng.action_mask(code=True).items()}
            ids = rng.permutation(B)[:max(1, B // 3)].astype(np.int32)
            for _ in range(3):
                eng.step(**_act(c, 30 + g))
            extras.update({"list." + n: t.clone() for n, t in eng.action_mask_boards(ids, code=True).items()})
            yield extras, True

    _twins(_mk(L, B, mode, multi, steps=40), drive, "masks %s %d" % (mode, L))


# ------------------------------------------------------------------ 8: episode accounting
def test_episode_accounting_inside_groups():
    """episode_stats(clear=True) and episode_records() inside the lagging groups every 10 steps:
    the sequence of counts and every record equal the twin's, each interval's sum of returns under
    streamutil.sum_tolerance, and the counts add up to the number of ``done`` seen.  ran_ahead:
    15 of 15 groups."""
    t, a = _twins(_mk(refill=4), _drive_rollout(120, stats_every=10), "episode accounting")
    for c in (t, a):
        counts = [int(x.item()) for x in c["counts"]]
        assert len(counts) == 12 and sum(counts) == int(c["dones"].sum().item()) and sum(counts) >= 4 * 33, counts
    assert [int(x.item()) for x in a["counts"]] == [int(x.item()) for x in t["counts"]]
    for x, y, n in zip(a["sums"], t["sums"], t["counts"]):
        assert abs(x.item() - y.item()) <= U.sum_tolerance(int(n.item())), (x.item(), y.item(), n.item())


# ------------------------------------------------------------------ 9: kernel timing
def test_kernel_timing_under_a_stream():
    """kernel_timing(8, 1), then eight steps and one copy_boards behind a spin on S: as many
    timed dispatches as the twin's run, every duration finite and positive (no bound on them:
    nothing has measured a step on a caller's stream).  ran_ahead: 1 of 1 group."""
    def drive(eng, c):
        eng.kernel_timing(8, 1)
        yield "lag"
        for k in range(8):
            eng.step(**_act(c, k))
        eng.copy_boards(np.array([0, 1], dtype=np.int32), np.array([5, 6], dtype=np.int32))
        yield {}, True
        c["times"] = eng.kernel_times()

    t, a = _twins(_mk(steps=8), drive, "kernel timing")
    assert len(t["times"]) == 8 and len(a["times"]) == len(t["times"])
    for times in (t["times"], a["times"]):
        assert np.isfinite(times).all() and (times > 0).all(), times.tolist()


# ------------------------------------------------------------------ 10: busy default stream
def test_rollout_with_a_busy_default_stream():
    """The rollout of test_rollout_autoreset (a refill every 4th step) with a spin on the default
    stream in front of every group as well: the trainer whose policy runs there.  ran_ahead: 15 of
    15 groups."""
    t, a = _twins(_mk(refill=4), _drive_rollout_final(120), "rollout, busy default stream", busy=True)
    _check_finished(t, a, 33)


def test_host_board_lists_with_a_busy_default_stream():
    """test_host_board_lists with a spin on the default stream in front of every group as well.
    ran_ahead: 1 of 1 asynchronous group."""
    _twins(_mk(), _drive_host_lists(), "host board lists, busy default stream", busy=True)


# ------------------------------------------------------------------ 11: two handles, two streams
def _drive_search(checkpoints=4):
    """step, copy_boards and step_boards_dev in turn, a "call" after each and a checkpoint after
    every tenth."""
    def drive(eng, c):
        rng = np.random.RandomState(19)
        B, k = eng.B, 0
        for _ in range(checkpoints):
            perm = rng.permutation(B)
            n = max(1, B // 4)
            dev_ids = torch.from_numpy(perm[:B // 2].astype(np.int32)).to(DEV)
            torch.cuda.synchronize()
            yield "lag"
            for j in range(10):
                if j % 3 == 0:
                    eng.step(**_act(c, k))
                elif j % 3 == 1:
                    eng.copy_boards(perm[:n].astype(np.int32), perm[n:2 * n].astype(np.int32))
                else:
                    eng.step_boards_dev(dev_ids, **_act(c, k))
                k += 1
                yield "call"
            yield {}, True
    return drive


def test_two_handles_on_two_streams():
    """A1 (TD-def 10x10, 33 boards) on S1 and A2 (TD-2p 20x20 multi-action, 9 boards) on S2, both
    with auto-reset, each issuing step, copy_boards and step_boards_dev calls; the host alternates
    between them call by call with a spin on both streams and synchronises nothing until a
    checkpoint every 10 calls.  Each equals its own twin, run alone on the default stream
    beforehand.  ran_ahead: 4 of 4 groups on both streams."""
    makes = [_mk(steps=40), _mk(20, 9, "2p", True, steps=40, seed0=2900)]
    twins = [_Run(m, _drive_search(), tag="two handles twin %d" % i).run().finish() for i, m in enumerate(makes)]
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    assert streams[0].cuda_stream != 0 and streams[1].cuda_stream not in (0, streams[0].cuda_stream)
    runs = [_Run(m, _drive_search(), stream=s, want=t.snaps, tag="two handles A%d" % (i + 1))
            for i, (m, s, t) in enumerate(zip(makes, streams, twins))]
    try:
        while not all(r.over for r in runs):
            ends = [r for r in runs if not r.over and r.advance()]
            for r in ends:  # (both streams were asked before the first snapshot waits for the device)
                r.settle()
    except BaseException:
        for r in runs:
            r.eng.close()
        raise
    errors = []
    for r in runs:
        try:
            r.finish()
        except AssertionError as e:  # (close both engines before reporting)
            errors.append(e)
    if errors:
        raise errors[0]


# ------------------------------------------------------------------ 12: made outside, run inside
def test_constructed_outside_the_stream():
    """A is constructed and reset on the default stream (its tensors were allocated there), then
    runs the rollout under S.  ran_ahead: 15 of 15 groups."""
    t, a = _twins(_mk(refill=4), _drive_rollout_final(120), "constructed outside", outside=True)
    _check_finished(t, a, 33)


# ------------------------------------------------------------------ 13: the caller's own streams
def _hip_runtime():
    """The HIP runtime torch has loaded (the one libtdstep.so is bound to), through ctypes."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no libamdhip64 in this process"
    hip = ctypes.CDLL(paths[0])
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    hip.hipStreamCreateWithFlags.restype = ctypes.c_int
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.restype = ctypes.c_int
    return hip


@pytest.mark.parametrize("flags", [0, 1], ids=["blocking", "non-blocking"])
def test_a_stream_the_caller_made(flags):
    """40 steps of the rollout on a stream made with hipStreamCreateWithFlags (0: a blocking
    stream, which the NULL stream synchronises with; 1: hipStreamNonBlocking) and wrapped as
    torch.cuda.ExternalStream.  ran_ahead: 5 of 5 groups on both."""
    hip = _hip_runtime()
    torch.cuda.synchronize()
    raw = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(raw), flags) == 0 and raw.value
    try:
        S = torch.cuda.ExternalStream(raw.value, device=DEV)
        _twins(_mk(refill=4, steps=40), _drive_rollout(40), "external stream flags=%d" % flags, stream=S)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(raw) == 0


# ------------------------------------------------------------------ 14: single-env and vector surfaces
def test_single_env_under_a_stream():
    """gym_TD.envs.TDDefense (host_io: pinned outputs, one stream synchronisation per step): 50
    steps under S, a spin in front of each, against a twin env on the default stream: the same
    observations, rewards, dones and infos.  Every step waits for the stream, so there is no
    asynchronous group here; ran_ahead is asked right after the spin was enqueued: 50 of 50."""
    acts = np.random.RandomState(23).randint(0, 601, size=50)
    seed = M.ok_seeds(10, 1, 31, O.MODE_DEF)[0][0]

    def play(before_step):
        env = E.TDDefense(10, seed=seed, opponent_seed=32)
        try:
            out = [("reset", env.reset())]
            for act in acts:
                before_step()
                r = env.step(int(act))
                out.append(("step", r[0], r[1:]))
                if r[2]:
                    out.append(("reset", env.reset()))
            assert (env._engine.flags() == 0).all()
            return out
        finally:
            env.close()

    want = play(lambda: None)
    S = torch.cuda.Stream(DEV)
    assert S.cuda_stream != 0
    ahead = []

    def spin():
        U.lag(S)
        ahead.append(bool(U.ran_ahead(S)))

    with torch.cuda.stream(S):
        got = play(spin)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and np.array_equal(g[1], w[1]) and g[2:] == w[2:], (k, g[2:], w[2:])
    print("single env: ran_ahead held behind %d of %d spins" % (sum(ahead), len(ahead)))
    assert len(ahead) == 50 and 2 * sum(ahead) >= 50


def test_vector_env_search_under_a_stream():
    """TDVecEnv(action_mask=True): 20 iterations of fork_dev + step_boards_dev (each followed by
    the mask kernels of refresh_action_mask) under S, in groups of five iterations: the same
    observations and masks as the twin's.  ran_ahead: 4 of 4 groups."""
    B = 33

    def make(c):
        vec = c["vec"] = E.TDVecEnv(10, B, "def", seed=4100, action_mask=True)
        vec.reset()
        c["acts"] = _acts(vec.engine, 20)
        return vec.engine

    def drive(eng, c):
        vec, rng = c["vec"], np.random.RandomState(29)
        for g in range(4):
            lists = []
            for _ in range(5):
                perm = rng.permutation(B)
                lists.append([torch.from_numpy(perm[i:j].astype(np.int32)).to(DEV) for i, j in ((0, 8), (8, 16))])
            torch.cuda.synchronize()
            yield "lag"
            for i, (src, dst) in enumerate(lists):
                vec.fork_dev(src, dst)
                _, _, _, infos = vec.step_boards_dev(dst, c["acts"][0][5 * g + i])
            yield dict(mask=infos["action_mask"].clone()), True

    _twins(make, drive, "vector env search")


# ------------------------------------------------------------------ 15: the oracle itself
def test_oracle_anchor_under_a_stream():
    """One anchor to the oracle, not the twin: TD-def 10x10, 16 boards, no auto-reset, 60 steps
    under S with a spin in front of each; every board goes through steputil.check_board against
    its oracle env at every step, as tests/test_gpu_envs.py does on the default stream.  The check
    reads the outputs, so every group is one step; ran_ahead right after the step: 60 of 60."""
    L, B, steps = 10, 16, 60
    seeds, orc = M.ok_seeds(L, B, 3100, O.MODE_DEF)
    rng = np.random.RandomState(L * 31 + 1)
    acts = np.array([[policies.discrete_def(rng, L, o._board.map[0], 0.5) for o in orc] for _ in range(steps)],
                    dtype=np.int64)
    S = torch.cuda.Stream(DEV)
    assert S.cuda_stream != 0
    ahead = 0
    with torch.cuda.stream(S):
        eng = TDEngine(L, B, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False)
        try:
            assert not eng.reset()[1]
            dev_acts = torch.from_numpy(acts).to(DEV)
            torch.cuda.synchronize()
            for k in range(steps):
                U.lag(S)
                eng.step(def_act=dev_acts[k])
                ahead += bool(U.ran_ahead(S))
                out = steputil.outputs(eng)
                for b, o in enumerate(orc):
                    if o._board.done():
                        continue
                    steputil.check_board(eng, out, b, o, o.step(int(acts[k, b]), None), "def", False, ("stream", k, b))
            assert (eng.flags() == 0).all() and eng.guard_timeouts() == 0
        finally:
            eng.close()
    print("oracle anchor: ran_ahead held for %d of %d steps" % (ahead, steps))
    assert 2 * ahead >= steps
