"""td_step_boards_dev / td_copy_boards_dev on the device: board lists, their length and their
validation in device memory.

The judge is a twin.  Engine A uses the device-list calls; engine B has the same seeds and
configuration and uses the host-list calls (td_step_boards / td_copy_boards, which the rest of the
suite pins to the oracle) with the same ids.  After every call the twins are compared byte for
byte over ALL boards, named or not: every output tensor (sentinels in the rows never written),
the exported state, both RNG streams, the flags, the episode records and the count of finished
episodes (the sum of their returns is an atomic float sum: see _sum_tolerance).  Small
handles throughout: 96 boards at L = 10, 48 at L = 20, 30 and 7.  Lists longer than one block of
the check kernel (2,100 boards) are in tests/test_gpu_board_lists_dev_blocks.py.  No test provokes a fault:
every bad list is one the check kernel is specified to catch, and on a bad verdict the consumer
reads no id.
"""
import numpy as np
import pytest
import torch

import maskutil as M

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import envs as E  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402

OUTPUTS = ("obs", "reward", "done", "win", "allow_next", "cooldowns", "ep_return", "ep_len", "real_def", "fail_def",
           "real_atk", "fail_atk")
SENTINEL = 0x5A
BOARDS = {10: 96, 20: 48, 30: 48, 7: 48}
DEV = torch.device("cuda", 0)
OK, BAD_COUNT, RANGE, TWICE, OVERLAP = range(5)


# ------------------------------------------------------------------ helpers
def _short(multi=False):
    """Episodes of at most 16 steps."""
    return M.hyper(multi, max_episode_steps=16)


def _engine(L, mode="def", multi=False, seed0=1700, sentinel=True, **kw):
    n = kw.pop("n", BOARDS[L])
    seeds = list(range(seed0, seed0 + n))
    kw.setdefault("retain_obs", False)
    eng = TDEngine(L, n, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, **kw)
    if L == 7:  # (no 7x7 map can be drawn: the boards start from caller layouts, maskutil.hand_layouts_7)
        recs = M.hand_layouts_7()
        eng.reset_layouts(np.stack([recs[b % 2] for b in range(n)]), np.arange(n, dtype=np.int32))
    else:
        eng.reset_all()
    if sentinel:  # rows no call writes keep a byte no step writes a whole row of
        for name in OUTPUTS:
            t = getattr(eng, name)
            if t is not None and not (name == "obs" and eng.retain_obs):  # (a retained buffer is the handle's)
                t.view(torch.uint8).fill_(SENTINEL)
    return eng


def _twins(L, **kw):
    return _engine(L, **kw), _engine(L, **kw)


def _draw(rng, eng):
    """Uniform random actions for every board, as device tensors (multi-action: sparse flags)."""
    L, n = eng.L, eng.B
    d = a = None
    if eng.mode != "atk":
        d = ((rng.random_sample((n, 6, L, L)) < 0.02).astype(np.int64) if eng.multi
             else rng.randint(0, 6 * L * L + 1, size=n).astype(np.int64))
        d = torch.from_numpy(d).to(DEV)
    if eng.mode != "def":
        a = torch.from_numpy(rng.randint(0, 5, size=(n, 3, 8)).astype(np.int64)).to(DEV)
    return dict(def_act=d, atk_act=a)


def _dev(ids):
    return torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(DEV)


def _snap(eng):
    """Everything the engine holds, as bytes."""
    torch.cuda.synchronize()
    s = {}
    for n in OUTPUTS:
        t = getattr(eng, n)
        if t is not None:
            s["out." + n] = t.view(torch.uint8).cpu().numpy().tobytes()
    for k, v in eng.export_state().items():
        s["state." + k] = np.ascontiguousarray(v).tobytes()
    s["flags"] = eng.flags().tobytes()
    s["np"] = b"".join(eng.get_np_state(b).tobytes() for b in range(eng.B))
    s["py"] = b"".join(np.asarray(eng.get_py_state(b)).tobytes() for b in range(eng.B))
    for k, t in zip(("ret", "len", "win"), eng.episode_records()):
        s["rec." + k] = t.cpu().numpy().tobytes()
    stats = eng.episode_stats().cpu().numpy()
    s["stats.n"] = stats[:1].tobytes()
    s[SUM] = float(stats[1])
    return s


# The one thing compared with a tolerance.  td_episode_stats' second word is a sum of doubles
# that the step kernels of either form accumulate with atomic adds, in the order the waves
# arrive: two runs of the SAME calls may differ in its last bits.  Two orders of summing n terms
# differ by at most 2 (n - 1) u sum|x_i|, u = 2^-53; a return is a sum of at most 1,200 rewards of
# at most reward_time + 128 reward_kill = 12.8 each, less at most base_LP penalty_leak = 50, so
# |x_i| < 1.6e4 under the default config.  The count beside it, and every board's own record
# (return, length, win), are compared byte for byte.
SUM = "stats.sum (atomic adds)"


def _sum_tolerance(n):
    return 2.0 * max(n - 1, 0) * 2.0 ** -53 * n * 1.6e4


def _assert_same(got, want, tag):
    assert set(got) == set(want)
    for k in want:
        if k != SUM:
            assert got[k] == want[k], (tag, k)
    n = int(np.frombuffer(want["stats.n"], dtype=np.float64)[0])
    assert abs(got[SUM] - want[SUM]) <= _sum_tolerance(n), (tag, SUM, got[SUM], want[SUM], n)


def _status():
    return torch.full((4,), -99, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ 1. step parity
@pytest.mark.parametrize("L,mode,multi,dtype", [(10, "def", False, torch.float32), (10, "atk", False, torch.float16),
                                                (20, "2p", True, torch.float32), (30, "def", False, torch.float32),
                                                (7, "def", False, torch.float32)])
def test_step_parity_with_the_host_list_twin(L, mode, multi, dtype):
    """48 calls; call t names the boards with (b + t) % 3 != 0, shuffled; every second call hands
    the list over through count_dev with cap = B and poison behind the count.  Every board is
    named 32 times and, with max_episode_steps = 16, finishes at least one episode through the
    list form's auto-reset.  (L = 7, the generic-side kernel: no 7x7 layout can be drawn, so there
    is nothing an auto-reset could stage; those boards run with auto-reset off and still finish
    their episode at step 16.)"""
    kw = dict(mode=mode, multi=multi, hp=_short(multi), obs_dtype=dtype, autoreset=L != 7)
    a, b = _twins(L, **kw)
    try:
        n_boards = a.B
        rng = np.random.RandomState(41)
        want_name = "td_step_list_kernel%s<%d, %d, %s>" % ("_f16" if dtype == torch.float16 else "",
                                                          L if L in (10, 20, 30) else 0,
                                                          {"def": 0, "atk": 1, "2p": 2}[mode], "true" if multi else "false")
        assert a.step_boards_dev_kernel_name() == want_name
        for t in range(48):
            ids = np.array([x for x in range(n_boards) if (x + t) % 3 != 0], dtype=np.int32)
            rng.shuffle(ids)
            acts = _draw(rng, a)
            st = _status()
            if t % 2:
                poison = [-7, n_boards + 5] + [int(ids[i % len(ids)]) for i in range(n_boards)]
                buf = np.concatenate([ids, np.asarray(poison, dtype=np.int32)])[:n_boards]
                a.step_boards_dev(_dev(buf), count=_dev([len(ids)]), status=st, **acts)
            else:
                a.step_boards_dev(_dev(ids), status=st, **acts)
            b.step_boards(ids, **acts)
            _assert_same(_snap(a), _snap(b), t)
            assert st.tolist() == [OK, t, -1, -1]
        length = a.episode_records()[1].cpu().numpy()  # (0 before a board's first finished episode)
        assert (length > 0).all(), "every board finished an episode through the list form's auto-reset"
        assert a.list_errors() == (0, None)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 2. copy parity
def _copy_cases(n_boards):
    root = 5
    kids = [x for x in range(n_boards) if x != root][10:41]
    perm = np.random.RandomState(3).permutation(n_boards)
    return {"fan-out": ([root] * 31, kids), "pairing": (perm[:40].tolist(), perm[40:80].tolist())}


@pytest.mark.parametrize("write_obs", [True, False])
@pytest.mark.parametrize("case", ["fan-out", "pairing"])
def test_copy_parity_with_the_host_list_twin(case, write_obs):
    a, b = _twins(10, autoreset=True)
    try:
        _copy_parity(a, b, case, write_obs)
    finally:
        a.close()
        b.close()


def test_copy_parity_random_agent_false():
    a, b = _twins(10, autoreset=False, random_agent=False)
    try:
        _copy_parity(a, b, "fan-out", True)
    finally:
        a.close()
        b.close()


def _copy_parity(a, b, case, write_obs):
    rng = np.random.RandomState(17)
    for _ in range(6):
        acts = _draw(rng, a)
        a.step(**acts)
        b.step(**acts)
    src, dst = _copy_cases(a.B)[case]
    st = _status()
    # through count_dev, with poison behind the count
    pad = a.B - len(src)
    a.copy_boards_dev(_dev(src + [-7] * pad), _dev(dst + [dst[0]] * pad), count=_dev([len(src)]), write_obs=write_obs,
                      status=st)
    b.copy_boards(src, dst, write_obs=write_obs)
    _assert_same(_snap(a), _snap(b), "copy")
    assert st.tolist() == [OK, 0, -1, -1]
    for k in range(3):
        acts = _draw(rng, a)
        a.step(**acts)
        b.step(**acts)
        _assert_same(_snap(a), _snap(b), ("step", k))


# ------------------------------------------------------------------ 3. a list built on the device
def test_not_done_list_built_on_the_device_without_a_sync():
    """"The boards that are not done", compacted with torch ops into a cap = B buffer with its
    count in a device tensor; the engine call runs under torch's sync-debug mode "error"."""
    kw = dict(hp=_short(), autoreset=True)
    a, b = _twins(10, **kw)
    try:
        n_boards = a.B
        rng = np.random.RandomState(5)
        even = np.arange(0, n_boards, 2, dtype=np.int32)
        acts = _draw(rng, a)
        a.step_boards_dev(_dev(even), **acts)
        b.step_boards(even, **acts)
        seen = set()
        for t in range(40):
            acts = _draw(rng, a)
            if t % 4 != 3:
                a.step(**acts)
                b.step(**acts)
                continue
            keep = a.done == 0
            buf = torch.argsort((~keep).to(torch.uint8), stable=True).to(torch.int32)
            count = keep.sum().to(torch.int32).reshape(1)
            st = _status()
            torch.cuda.synchronize()
            old = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                a.step_boards_dev(buf, count=count, status=st, **acts)
            finally:
                torch.cuda.set_sync_debug_mode(old)
            n = int(count.item())
            seen.add(n)
            b.step_boards(buf[:n].cpu().numpy(), **acts)
            _assert_same(_snap(a), _snap(b), t)
            assert st[0].item() == OK
        assert any(0 < n < n_boards for n in seen), seen
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 4. device refusals
def _refusals(n_boards):
    """(kind, args, count, code, allowed entries, board, the valid follow-up naming the same boards)"""
    return [
        ("step", [list(range(10))], -1, BAD_COUNT, {-1}, -1, ("step", [list(range(10))])),
        ("step", [list(range(10))], 11, BAD_COUNT, {-1}, 11, ("step", [list(range(10))])),
        ("step", [[3, 4, 5, -1]], None, RANGE, {3}, -1, ("step", [[3, 4, 5]])),
        ("copy", [[n_boards, 1], [2, 3]], None, RANGE, {0}, n_boards, ("copy", [[1, 1], [2, 3]])),
        ("step", [[5, 6, 5]], None, TWICE, {0, 2}, 5, ("step", [[5, 6]])),
        ("copy", [[1, 2], [7, 7]], None, TWICE, {0, 1}, 7, ("copy", [[1, 2], [7, 9]])),
        ("copy", [[1, 2], [3, 1]], None, OVERLAP, {0, 1}, 1, ("copy", [[2, 3], [1, 4]])),
    ]


def test_device_refusals_change_nothing_and_the_next_call_works():
    a = _engine(10, autoreset=True, retain_obs=True)
    b = _engine(10, autoreset=True, retain_obs=True)
    try:
        rng = np.random.RandomState(23)
        for _ in range(4):
            acts = _draw(rng, a)
            a.step(**acts)
            b.step(**acts)
        serial = 0
        for kind, args, count, code, entries, board, (okind, oargs) in _refusals(a.B):
            tag = (kind, args, count)
            before = _snap(a)
            st = _status()
            acts = _draw(rng, a)
            cnt = None if count is None else _dev([count])
            if kind == "step":
                a.step_boards_dev(_dev(args[0]), count=cnt, status=st, **acts)
            else:
                a.copy_boards_dev(_dev(args[0]), _dev(args[1]), count=cnt, status=st)
            torch.cuda.synchronize()
            _assert_same(_snap(a), before, tag)
            got = st.tolist()
            assert got[0] == code and got[1] == serial and got[2] in entries and got[3] == board, (tag, got)
            n, first = a.list_errors()
            assert n == 1 and first == dict(code=code, call=serial, entry=got[2], board=board), (tag, n, first)
            assert a.list_errors() == (0, None)
            serial += 1
            # the valid call that names the very boards the bad list named
            st = _status()
            if okind == "step":
                a.step_boards_dev(_dev(oargs[0]), status=st, **acts)
                b.step_boards(oargs[0], **acts)
            else:
                a.copy_boards_dev(_dev(oargs[0]), _dev(oargs[1]), status=st)
                b.copy_boards(oargs[0], oargs[1])
            _assert_same(_snap(a), _snap(b), ("after", tag))
            assert st.tolist() == [OK, serial, -1, -1], (tag, st.tolist())
            serial += 1
        assert a.list_errors() == (0, None)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 5. back to back
def _script(rng, n_boards, calls=40):
    """Alternating step / copy calls with varying lists; calls 13 and 26 are refused lists."""
    out = []
    for t in range(calls):
        perm = rng.permutation(n_boards).astype(np.int32)
        k = int(rng.randint(1, n_boards // 2))
        if t % 2 == 0:
            ids = perm[:k].tolist()
            if t == 26:
                ids = ids + [ids[0]]  # a board twice
            out.append(("step", ids, None, t == 26))
        else:
            src, dst = perm[:k].tolist(), perm[k:2 * k].tolist()
            if t == 13:
                dst[-1] = src[0]  # a board in both
            out.append(("copy", src, dst, t == 13))
    return out


def _run_script(eng, script, acts, device_lists, sync):
    for (kind, x, y, bad), act in zip(script, acts):
        if kind == "step":
            if device_lists:
                eng.step_boards_dev(_dev(x), **act)
            elif not bad:
                eng.step_boards(x, **act)
        else:
            if device_lists:
                eng.copy_boards_dev(_dev(x), _dev(y), write_obs=True)
            elif not bad:
                eng.copy_boards(x, y, write_obs=True)
        if sync:
            torch.cuda.synchronize()


def test_forty_calls_back_to_back():
    """No synchronisation between the calls: the scratch and the verdict are handed over between
    consecutive check / consumer kernels in stream order alone."""
    kw = dict(hp=_short(), autoreset=True)
    engines = [_engine(10, **kw) for _ in range(3)]
    try:
        rng = np.random.RandomState(77)
        script = _script(rng, engines[0].B)
        acts = [_draw(rng, engines[0]) for _ in script]
        torch.cuda.synchronize()
        _run_script(engines[0], script, acts, True, False)
        _run_script(engines[1], script, acts, True, True)
        _run_script(engines[2], script, acts, False, True)
        snaps = [_snap(e) for e in engines]
        _assert_same(snaps[0], snaps[1], "no sync vs sync")
        _assert_same(snaps[0], snaps[2], "device lists vs host lists")
        for e in engines[:2]:
            n, first = e.list_errors()
            assert n == 2 and first["call"] == 13 and first["code"] == OVERLAP, (n, first)
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------ 6. retained buffer
def test_retained_buffer_always_equals_a_twin_that_writes_every_byte():
    a = _engine(10, sentinel=False, autoreset=True, retain_obs=True)
    b = _engine(10, sentinel=False, autoreset=True, retain_obs=False)
    try:
        assert a.retain_obs and not b.retain_obs
        rng = np.random.RandomState(9)
        plan = ["step", "step", "list", "list", "step", "copy+", "list", "step", "step", "copy-", "list", "step", "copy+",
                "copy-", "step", "list", "copy+", "step", "step", "list"]
        for t, what in enumerate(plan):
            acts = _draw(rng, a)
            perm = rng.permutation(a.B).astype(np.int32)
            k = int(rng.randint(1, a.B // 2))
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


# ------------------------------------------------------------------ 7. host refusals
def test_host_refusals_with_a_live_handle():
    plain = _engine(10, n=8, autoreset=True)
    skip = _engine(10, n=8, autoreset=True, frame_skip=2)
    npa = _engine(10, n=8, autoreset=True, random_agent=False)
    try:
        rng = np.random.RandomState(2)
        for eng, ids, word in ((plain, list(range(8)) + [0], "cap = 9"), (skip, [1, 2], "frame skip"),
                               (npa, [1, 2], "random_agent")):
            before = _snap(eng)
            acts = _draw(rng, eng)
            with pytest.raises(_lib.TDError) as err:
                eng.step_boards_dev(_dev(ids), **acts)
            assert word in str(err.value) and "td_step_boards_dev" in str(err.value)
            _assert_same(_snap(eng), before, word)
            assert eng.list_errors() == (0, None)
        before = _snap(plain)
        with pytest.raises(_lib.TDError) as err:
            plain.copy_boards_dev(_dev(list(range(9))), _dev(list(range(9))))
        assert "td_copy_boards_dev: cap = 9" in str(err.value)
        _assert_same(_snap(plain), before, "copy cap")
        # ids on the host belong to the host-list methods
        for bad in ([1, 2], np.array([1, 2], dtype=np.int32), torch.tensor([1, 2], dtype=torch.int32)):
            with pytest.raises(ValueError, match="step_boards"):
                plain.step_boards_dev(bad, **_draw(rng, plain))
            with pytest.raises(ValueError, match="copy_boards"):
                plain.copy_boards_dev(bad, _dev([3, 4]))
        # an int64 device tensor is converted on the device; an empty list is a no-op
        acts = _draw(rng, plain)
        plain.step_boards_dev(torch.tensor([1, 2], dtype=torch.int64, device=DEV), **acts)
        plain.step_boards_dev(_dev([]), **acts)
        assert plain.list_errors() == (0, None)
    finally:
        plain.close()
        skip.close()
        npa.close()


# ------------------------------------------------------------------ 8. vector env
def test_vector_env_fork_dev_step_boards_dev_and_masks():
    """One search iteration: fork the root into the leaves, step the leaves, read their masks."""
    env = E.TDVecEnv(10, 16, "def", seed=300, autoreset=False, action_mask=True)
    twin = E.TDVecEnv(10, 16, "def", seed=300, autoreset=False, action_mask=True)
    try:
        env.reset()
        twin.reset()
        rng = np.random.RandomState(6)
        for _ in range(5):
            a = torch.from_numpy(rng.randint(0, 601, size=16).astype(np.int64)).to(DEV)
            env.step(a)
            twin.step(a)
        src, dst = [4, 4, 4], [9, 2, 3]
        st = _status()
        o = env.fork_dev(_dev(src), _dev(dst), status=st)
        wo = twin.fork(src, dst)
        assert o is env.engine.obs and torch.equal(o, wo)
        assert torch.equal(env.action_masks()["def"], twin.action_masks()["def"])
        for _ in range(5):
            a = torch.from_numpy(rng.randint(0, 601, size=16).astype(np.int64)).to(DEV)
            o, r, dn, info = env.step_boards_dev(_dev(dst), a, status=st)
            wo, wr, wd, winfo = twin.step_boards(dst, a)
            assert set(info) == set(winfo)
            for got, want in ((o, wo), (r, wr), (dn, wd), (info["action_mask"], winfo["action_mask"]),
                              (info["RealAction"], winfo["RealAction"])):
                assert torch.equal(got, want)
            assert st[0].item() == OK
        assert torch.equal(info["action_mask"], env.engine.action_mask()["def"])
        assert env.engine.list_errors() == (0, None)
    finally:
        env.close()
        twin.close()
