"""Frame skip on the device (td_set_frame_skip, the td_skip_kernel family): one td_step runs
up to k board steps per board and writes one observation.

The reference is the env stepped sub-step by sub-step (skiputil.Ref: oracle.td_cpu.Env for the
bytes, oracle.td_oracle.Env beside it for the info fields), stopped at ``done``, reset with
the next layout draw that succeeds, rewards summed left to right in f64.  Everything is
compared bit for bit.  tests/test_frame_skip_ref.py shows on the CPU that the recipe ends at
least 5 episodes at every sub-step position, so a pass here means the early-stop branch ran
at each of them."""
import copy
import functools

import numpy as np
import pytest
import torch

import maskutil as M
import skiputil as S
from oracle import canon

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import envs as E  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402

lib = _lib.lib


# ------------------------------------------------------------------ helpers
def _engine(L, seeds, mode, cfg, hp=None, **kw):
    eng = TDEngine(L, len(seeds), mode, False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, cfg=cfg, hp=hp, **kw)
    _, failed = eng.reset()
    assert not failed
    return eng


def _step(eng, acts):
    d, a = acts
    eng.step(def_act=None if d is None else torch.from_numpy(d), atk_act=None if a is None else torch.from_numpy(a))


def _empty(eng):
    d = np.full(eng.B, 6 * eng.L * eng.L, dtype=np.int64) if eng.mode != "atk" else None
    a = np.full((eng.B, 3, 8), 4, dtype=np.int64) if eng.mode != "def" else None
    return d, a


def _phase_shift(eng, k):
    """Board b takes b % k empty single steps (at frame skip 1): the engine steps all boards
    together, so the batch is put together from the states after 0 .. k-1 steps."""
    assert eng.frame_skip == 1
    states = [eng.export_state()]
    for _ in range(k - 1):
        _step(eng, _empty(eng))
        assert not bool(eng.done.any()), "an episode ended during the phase shift"
        states.append(eng.export_state())
    eng.import_state({name: np.concatenate([states[b % k][name][b:b + 1] for b in range(eng.B)])
                      for name in states[0]})


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


class Trace(object):
    """A reference run: per macro step the actions and every board's expected outputs, and
    every 10th step the state digests."""

    def __init__(self, mode, k, L=10, B=S.RECIPE_BOARDS, steps=S.RECIPE_STEPS, cfg=None, ks=None):
        self.mode, self.L, self.cfg = mode, L, cfg or S.recipe_cfg()
        self.k0 = k
        self.ks = ks or [k] * steps  # frame skip of every macro step
        self.seeds, refs = S.make_refs(L, B, mode, self.cfg)
        try:
            self.first = [r.obs() for r in refs]
            for b, ref in enumerate(refs):
                for _ in range(b % k):
                    assert not ref.macro(1)["done"]
            rng = np.random.RandomState(1)
            self.acts, self.outs, self.digests = [], [], {}
            for i, ki in enumerate(self.ks):
                acts = S.draw_actions(rng, mode, B, L)
                self.acts.append(acts)
                self.outs.append([ref.macro(ki, *S.act_of(acts, b)) for b, ref in enumerate(refs)])
                if i % 10 == 9:
                    self.digests[i] = [canon.digest(r.state_bytes()) for r in refs]
        finally:
            for r in refs:
                r.close()

    def ends(self):
        e = np.zeros(max(self.ks), dtype=int)
        for row in self.outs:
            for o in row:
                if o["done"]:
                    e[o["ran"] - 1] += 1
        return e


@functools.lru_cache(maxsize=1)
def _trace_def4():
    """The TD-def k = 4 recipe run, shared by the parity, float16 and retention cases."""
    return Trace("def", 4)


def _compare(eng, outs, where, f16=False):
    ob = eng.obs.cpu().numpy()
    host = {n: getattr(eng, n).cpu().numpy() for n in ("reward", "done", "win", "allow_next", "cooldowns", "ep_return", "ep_len")}
    for n in ("real_def", "fail_def", "real_atk", "fail_atk"):
        t = getattr(eng, n)
        host[n] = None if t is None else t.cpu().numpy()
    for b, o in enumerate(outs):
        if o is None:  # (a board the caller compares by itself)
            continue
        w = (where, b, o["ran"])
        want = np.asarray(o["obs"], dtype=np.float32)
        want = want.astype(np.float16) if f16 else want
        assert np.array_equal(_bits(ob[b]), _bits(want)), (w, "obs", np.argwhere(_bits(ob[b]) != _bits(want))[:5].tolist())
        assert canon.fhex(host["reward"][b]) == canon.fhex(o["reward"]), (w, "reward")
        assert bool(host["done"][b]) == o["done"], (w, "done")
        assert int(host["win"][b]) == o["win"], (w, "win")
        assert int(host["allow_next"][b]) == o["allow"], (w, "allow_next")
        assert int(host["cooldowns"][b]) == o["cool"], (w, "cooldowns")
        assert canon.fhex(host["ep_return"][b]) == canon.fhex(o["ep_ret"]), (w, "ep_return")
        assert int(host["ep_len"][b]) == o["ep_len"], (w, "ep_len")
        if eng.mode != "atk":  # sub-step 0's
            assert int(host["real_def"][b]) == o["real_def"], (w, "real_def")
            assert int(host["fail_def"][b]) == o["fail_def"], (w, "fail_def")
        if eng.mode != "def":
            assert np.array_equal(host["real_atk"][b], o["real_atk"]), (w, "real_atk")
            assert np.array_equal(host["fail_atk"][b], o["fail_atk"]), (w, "fail_atk")


def _play(eng, tr, f16=False):
    """Phase-shift the engine, then run the trace's macro steps on it and compare."""
    _phase_shift(eng, tr.k0)
    for i, (ki, acts, outs) in enumerate(zip(tr.ks, tr.acts, tr.outs)):
        if eng.frame_skip != ki:
            eng.set_frame_skip(ki)
        _step(eng, acts)
        _compare(eng, outs, (tr.mode, ki, i), f16)
        if i in tr.digests:
            st = eng.export_state()
            for b in range(eng.B):
                assert canon.state_digest(eng.board_state(b, st)) == tr.digests[i][b], ("state", tr.mode, ki, i, b)
    assert (eng.flags() == 0).all()


def _run(tr, f16=False, **kw):
    eng = _engine(tr.L, tr.seeds, tr.mode, tr.cfg, **kw)
    try:
        ob = eng.obs.cpu().numpy()
        for b, w in enumerate(tr.first):
            assert np.array_equal(_bits(ob[b]), _bits(w.astype(np.float16) if f16 else w)), ("first obs", b)
        _play(eng, tr, f16)
    finally:
        eng.close()


# ------------------------------------------------------------------ 1 parity
@pytest.mark.parametrize("mode,k", S.RECIPE_CASES)
def test_parity_with_the_reference_recipe(mode, k):
    tr = _trace_def4() if (mode, k) == ("def", 4) else Trace(mode, k, steps=S.recipe_steps(mode, k))
    S.check_ends(mode, k, tr.ends())  # (tests/test_frame_skip_ref.py, on the C oracle alone)
    if mode == "def" or k == 3:
        assert (tr.ends() >= 5).all(), tr.ends()
    _run(tr)


@pytest.mark.parametrize("mode", ["def", "atk", "2p"])
def test_parity_with_cool_downs(mode):
    """Action intervals of 2 and 3: sub-steps in which a side is still cooling down -- the
    built-in opponent draws nothing there, and the TD-atk kernel keeps its packed cells."""
    _run(Trace(mode, 3, cfg=S.recipe_cfg(attacker_action_interval=2, defender_action_interval=3)))


# ------------------------------------------------------------------ 2 other sides
FAST = [[.9, .9], [.7, .7], [.6, .6], [.6, .6]]  # enemy_speed


@pytest.mark.parametrize("L,k", [(20, 4), (30, 4), (12, 3), (11, 3)])
def test_other_sides(L, k):
    """20 and 30: the other two line-writer builds; 12 and 11: the generic build's quad and
    per-element observation paths.  (Faster enemies: episodes end inside 20 macro steps on the
    longer roads too.)"""
    tr = Trace("def", k, L=L, B=16, steps=20, cfg=S.recipe_cfg(enemy_speed=FAST))
    assert tr.ends().sum() >= 5, tr.ends()
    _run(tr)


@pytest.mark.parametrize("L", [20, 11])
def test_other_sides_attacker(L):
    """TD-atk beside the above: the kernel that keeps the raw cell words aside."""
    tr = Trace("atk", 3, L=L, B=16, steps=20, cfg=S.recipe_cfg(enemy_speed=FAST))
    assert tr.ends().sum() >= 5, tr.ends()
    _run(tr)


# ------------------------------------------------------------------ 3 float16
def test_float16_observation():
    _run(_trace_def4(), f16=True, obs_dtype=torch.float16)


# ------------------------------------------------------------------ 4 retention
@pytest.mark.parametrize("retain", [True, False])
def test_retained_observation(retain):
    """Both engines equal the oracle byte for byte, hence each other: with retention "before"
    is the board as loaded at the start of the macro step."""
    tr = _trace_def4()
    eng = _engine(tr.L, tr.seeds, tr.mode, tr.cfg, retain_obs=retain)
    try:
        assert (lib.td_retained_obs(eng._h) == eng.obs.data_ptr()) == eng.retain_obs
        assert eng.retain_obs == (retain and _retain_enabled())
        _play(eng, tr)
    finally:
        eng.close()


def _retain_enabled():
    from gym_TD import engine
    return engine.RETAIN_OBS


# ------------------------------------------------------------------ 5 unaligned buffers
def _run_into(buf, off, nbytes, dtype, L, n, steps, k):
    seeds = 900 + np.arange(n)
    eng = TDEngine(L, n, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, obs_dtype=dtype, frame_skip=k)
    try:
        eng.obs = buf[off:off + nbytes].view(dtype).view(n, 45, L, L)
        eng._io.obs = eng.obs.data_ptr()
        assert eng.obs.data_ptr() == buf.data_ptr() + off
        eng.reset_all()
        out = []
        g = torch.Generator(device="cuda").manual_seed(3)
        for _ in range(steps):
            eng.step(def_act=torch.randint(0, 6 * L * L + 1, (n,), device="cuda", generator=g, dtype=torch.int64))
            out.append(buf[off:off + nbytes].clone())
        assert (eng.flags() == 0).all()
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_obs_stays_inside_an_unaligned_buffer(dtype):
    """The observation at +0, +8 and +2 bytes inside a buffer of 0xA5 (float16: the line writer
    at the other 8-B phase, and the per-element path; float32, whose pointer must be
    element-aligned: +8 and +4, both the per-element path): the same board bytes, not a byte
    outside them."""
    L, n, steps, pad, k = 10, 33, 8, 1024, 4
    nbytes = n * 45 * L * L * (4 if dtype == torch.float32 else 2)
    ref = None
    for shift in (0, 8, 2 if dtype == torch.float16 else 4):
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 128 == 0
        out = _run_into(buf, pad + shift, nbytes, dtype, L, n, steps, k)
        guard = torch.cat([buf[:pad + shift], buf[pad + shift + nbytes:]])
        assert bool((guard == 0xA5).all()), ("bytes outside the boards were written", shift)
        if ref is None:
            ref = out
            assert not bool((ref[-1] == 0xA5).all())
        else:
            for i, (x, y) in enumerate(zip(out, ref)):
                assert torch.equal(x, y), ("board bytes differ from the run at offset 0", shift, i)


# ------------------------------------------------------------------ 6 live switch
def test_live_switch():
    """k goes 1 -> 4 -> 1 -> 3 on a running engine."""
    ks = [1] * 12 + [4] * 12 + [1] * 12 + [3] * 12
    tr = Trace("def", 1, ks=ks)
    assert sum(o["done"] for row in tr.outs for o in row) > 20
    eng = _engine(tr.L, tr.seeds, tr.mode, tr.cfg)
    try:
        _play(eng, tr)
        assert eng.frame_skip == 3 and lib.td_frame_skip(eng._h) == 3
    finally:
        eng.close()


# ------------------------------------------------------------------ 7 equivalence on the device
def _live(st):
    """The exported arrays with the slots beyond n_en / n_tw zeroed."""
    st = {k: v.copy() for k, v in st.items()}
    for names, n, cap in ((("en_lp", "en_mg", "en_inf"), st["hdr"]["n_en"], _lib.ECAP),
                          (("tw_cd", "tw_inf"), st["hdr"]["n_tw"], _lib.TCAP)):
        dead = np.arange(cap)[None, :] >= n[:, None]
        for name in names:
            st[name][dead] = 0
    return st


@pytest.mark.parametrize("mode", ["def", "atk"])
def test_macro_step_equals_k_single_steps_on_the_device(mode):
    """Default-config boards (no episode ends in 40 board steps): a k = 4 engine against k = 1
    twins taking (action, empty, empty, empty).  The raw export carries the opponent stream's
    lazy-twist boundary, which follows how far a kernel pre-draws: the skip kernel pre-draws as
    td_step_kernel does, so the twin on the large kernel is equal word for word; the twin on
    the kernel td_create chose is compared through get_py_state, the stream's canonical form.
    (Slots of the enemy and tower arrays beyond the live counts are no state: a step leaves there
    what an earlier, longer list held, and a macro step stores the list once.)"""
    L, B, k = 10, 16, 4
    seeds, refs = S.make_refs(L, B, mode, S.O.Config(), info=False)
    for r in refs:
        r.close()
    a = TDEngine(L, B, mode, False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, frame_skip=k)
    twins = [TDEngine(L, B, mode, False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, step_kernel=kind)
             for kind in ("large", "auto")]
    try:
        for e in [a] + twins:
            _, failed = e.reset()
            assert not failed
        rng = np.random.RandomState(5)
        for i in range(10):
            acts = S.draw_actions(rng, mode, B, L)
            _step(a, acts)
            sa = _live(a.export_state())
            for t, exact in zip(twins, (True, False)):
                tot = None
                for j in range(k):
                    _step(t, acts if j == 0 else _empty(t))
                    assert not bool(t.done.any())
                    r = t.reward.cpu().numpy().copy()
                    tot = r if j == 0 else tot + r
                assert np.array_equal(a.reward.cpu().numpy().view(np.uint64), tot.view(np.uint64)), i
                assert not bool(a.done.any())
                assert np.array_equal(_bits(a.obs.cpu().numpy()), _bits(t.obs.cpu().numpy())), i
                st = _live(t.export_state())
                for name in sa:
                    if exact or name != "opp_mt":
                        assert np.array_equal(sa[name], st[name]), (i, name, exact)
                for b in range(4):
                    assert np.array_equal(a.get_py_state(b), t.get_py_state(b)), (i, b)
    finally:
        for e in [a] + twins:
            e.close()


# ------------------------------------------------------------------ 8 step-limit end
def test_step_limit_end():
    """max_episode_steps = 10 at k = 4: the third macro step runs 2 sub-steps and ends the
    episode at its step limit; the fourth starts the new one."""
    L, B, k = 10, 8, 4
    hp = M.hyper(False, max_episode_steps=10)
    cfg = S.O.Config()
    seeds, refs = S.make_refs(L, B, "def", cfg, c_env=False, hp=hp)
    eng = _engine(L, seeds, "def", cfg, hp=hp, frame_skip=k)
    try:
        rng = np.random.RandomState(2)
        for i in range(5):
            acts = S.draw_actions(rng, "def", B, L)
            outs = [ref.macro(k, *S.act_of(acts, b)) for b, ref in enumerate(refs)]
            _step(eng, acts)
            _compare(eng, outs, ("limit", i))
            if i == 2:
                assert all(o["ran"] == 2 and o["done"] and o["ep_len"] == 10 for o in outs)
                assert (eng.ep_len.cpu().numpy() == 10).all() and bool(eng.done.all())
                assert (eng.win.cpu().numpy() == 1).all()  # the base stood
            else:
                assert all(o["ran"] == 4 and not o["done"] for o in outs)
            st = eng.export_state()
            assert (st["hdr"]["steps"] == (0 if i == 2 else 4 * (i + 1) if i < 2 else 4 * (i - 2))).all()
            for b, ref in enumerate(refs):
                assert canon.state_digest(eng.board_state(b, st)) == canon.state_digest(canon.oracle_state(ref.o)), (i, b)
        assert (eng.flags() == 0).all()
    finally:
        eng.close()


# ------------------------------------------------------------------ 8b td_set_config between macro steps
@pytest.mark.parametrize("autoreset", [False, True])
def test_set_config_between_macro_steps(autoreset):
    """A new config before every macro step of 3 (skiputil.ConfigTrace): the enemies and towers
    created in sub-steps 1 and 2 capture the launch's config epoch as those of sub-step 0 do,
    and with auto-reset an episode that ends inside a macro step starts the next one under
    that launch's config.  The state digest carries each entity's captured values."""
    from gym_TD import params as P
    tr = S.ConfigTrace(autoreset)
    tr.check()  # (tests/test_frame_skip_ref.py, without a GPU)
    eng = TDEngine(tr.L, len(tr.seeds), "def", False, 1, np_seeds=tr.seeds, py_seeds=tr.seeds, autoreset=autoreset,
                   cfg=tr.cfg(0, copy.deepcopy(P.config)), frame_skip=tr.k)
    try:
        _, failed = eng.reset()
        assert not failed
        ob = eng.obs.cpu().numpy()
        for b, w in enumerate(tr.first):
            assert np.array_equal(_bits(ob[b]), _bits(w)), ("first obs", b)
        for i, (acts, outs) in enumerate(zip(tr.acts, tr.outs)):
            eng.set_config(tr.cfg(i + 1, copy.deepcopy(P.config)))
            eng.step(def_act=torch.from_numpy(acts))
            ob, rw, dn = eng.obs.cpu().numpy(), eng.reward.cpu().numpy(), eng.done.cpu().numpy()
            real, fail = eng.real_def.cpu().numpy(), eng.fail_def.cpu().numpy()
            st = eng.export_state()
            for b, o in enumerate(outs):
                if o is None:  # (finished in an earlier macro step, no auto-reset)
                    continue
                w = (autoreset, i, b, o["ran"])
                assert canon.fhex(rw[b]) == canon.fhex(o["reward"]) and bool(dn[b]) == o["done"], w
                assert canon.state_digest(eng.board_state(b, st)) == o["digest"], w
                assert np.array_equal(_bits(ob[b]), _bits(np.asarray(o["obs"], dtype=np.float32))), w
                assert int(real[b]) == o["real_def"] and int(fail[b]) == o["fail_def"], w
        assert (eng.flags() == 0).all()
    finally:
        eng.close()


# ------------------------------------------------------------------ 8c boards never reset
NEVER_K, NEVER_B, NEVER_STEPS = 4, 32, 6
FLAG_NO_LAYOUT = 8  # include/tdstep.h td_board_flag


@pytest.mark.parametrize("L,dtype,garbage", [(L, dt, False) for L in (10, 20) for dt in (torch.float32, torch.float16)]
                         + [(10, torch.float32, True), (20, torch.float32, True)])
def test_boards_never_reset(L, dtype, garbage):
    """skip_board's own copy of the "never reset" branch: 32 boards with every seed of the
    road table whose first draw fails (L = 10: 8 of them; the table has none at L = 20) and two
    boards the caller left out of reset().  At frame skip 4 such a board shows, every macro step,
    an all-zero observation, done 1, win -1, reward +0.0, nothing allowed, the empty action
    back, flag word exactly TD_FLAG_NO_LAYOUT and the state the reset left; the healthy boards
    beside it are the reference's.  garbage: the observation buffer holds 0xA5 before the
    reset, with retention on -- the windows of those boards are written, not skipped."""
    import goldens as G
    rows = G.load_roadgen()[str(L)]
    err = sorted(int(s) for s in rows if "err" in rows[s])[:8]
    good = sorted(int(s) for s in rows if "err" not in rows[s])[:NEVER_B - len(err)]
    seeds = sorted(err + good)
    left_out = [3, 17]
    assert all(seeds[b] in good for b in left_out) and (len(err) == 8 or L != 10)
    never = sorted([b for b, s in enumerate(seeds) if s in err] + left_out)
    f16 = dtype == torch.float16
    cfg = S.recipe_cfg()
    refs = [None if b in never else S.Ref(L, "def", s, cfg) for b, s in enumerate(seeds)]
    eng = TDEngine(L, NEVER_B, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, cfg=cfg,
                   obs_dtype=dtype, retain_obs=True, frame_skip=NEVER_K)
    try:
        assert eng.retain_obs == _retain_enabled()
        if garbage:
            eng.obs.view(torch.uint8).fill_(0xA5)
        mask = np.ones(NEVER_B, dtype=np.uint8)
        mask[left_out] = 0
        _, failed = eng.reset(mask)
        assert sorted(failed) == [b for b, s in enumerate(seeds) if s in err], (failed, err)
        st0 = eng.export_state()
        assert (st0["hdr"]["num_roads"][never] == 0).all() and (st0["hdr"]["flags"] == 0).all()
        if garbage:
            assert bool((eng.obs[never].view(torch.uint8) == 0xA5).all())
        rng = np.random.RandomState(4)
        empty = 6 * L * L
        for i in range(NEVER_STEPS):
            acts = S.draw_actions(rng, "def", NEVER_B, L)
            outs = [None if r is None else r.macro(NEVER_K, *S.act_of(acts, b)) for b, r in enumerate(refs)]
            _step(eng, acts)
            _compare(eng, outs, ("never", L, i), f16)
            assert not bool(eng.obs[never].view(torch.uint8).any()), i  # every byte zero
            host = {n: getattr(eng, n).cpu().numpy()[never] for n in
                    ("reward", "done", "win", "allow_next", "cooldowns", "real_def", "fail_def", "ep_return", "ep_len")}
            assert (host["reward"].view(np.uint64) == 0).all() and (host["ep_return"].view(np.uint64) == 0).all(), i
            assert (host["done"] == 1).all() and (host["win"] == -1).all(), i
            for n in ("allow_next", "cooldowns", "fail_def", "ep_len"):
                assert (host[n] == 0).all(), (i, n)
            assert (host["real_def"] == empty).all(), i
            flags = eng.flags()
            assert (flags[never] == FLAG_NO_LAYOUT).all() and flags.sum() == FLAG_NO_LAYOUT * len(never), (i, flags.tolist())
            st = eng.export_state()
            for name in st0:
                if name == "hdr":
                    for f in st0["hdr"].dtype.names:
                        if f != "flags":
                            assert np.array_equal(st["hdr"][f][never], st0["hdr"][f][never]), (i, f)
                else:
                    assert np.array_equal(st[name][never], st0[name][never]), (i, name)
    finally:
        eng.close()
        for r in refs:
            if r is not None:
                r.close()


# ------------------------------------------------------------------ 9 refusals
def _refused(h, k, before):
    assert lib.td_set_frame_skip(h, k) < 0
    assert lib.td_last_error().decode()
    assert lib.td_frame_skip(h) == before


def test_refusals_change_nothing():
    seeds = np.arange(4) + 500
    plain = TDEngine(10, 4, "def", False, 1, np_seeds=seeds, py_seeds=seeds)
    multi = TDEngine(10, 4, "def", True, 1, np_seeds=seeds, py_seeds=seeds)
    fixed = TDEngine(10, 4, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, random_agent=False)
    try:
        _refused(plain._h, 0, 1)
        _refused(plain._h, 17, 1)
        _refused(multi._h, 2, 1)
        _refused(fixed._h, 2, 1)
        assert lib.td_set_frame_skip(multi._h, 1) == 0 and lib.td_set_frame_skip(fixed._h, 1) == 0  # k = 1 is always fine
        plain.set_frame_skip(2)
        name = plain.step_kernel_name
        assert lib.td_set_random_agent(plain._h, 0) < 0
        assert "frame skip" in lib.td_last_error().decode()
        assert lib.td_frame_skip(plain._h) == 2 and plain.step_kernel_name == name
        _refused(plain._h, 17, 2)
        # the Python surface: ValueError for what is no frame skip, TDError for what the handle refuses
        with pytest.raises(ValueError, match="frame_skip"):
            plain.set_frame_skip(0)
        with pytest.raises(_lib.TDError):
            multi.set_frame_skip(2)
        assert multi.frame_skip == 1
        with pytest.raises(_lib.TDError):
            TDEngine(10, 4, "def", True, 1, frame_skip=2)
        # and the engine that refused still steps (random_agent is still True on `plain`)
        plain.reset_all()
        plain.step(def_act=torch.full((4,), 600, dtype=torch.int64))
        assert (plain.export_state()["hdr"]["steps"] == 2).all()
    finally:
        for e in (plain, multi, fixed):
            e.close()


# ------------------------------------------------------------------ 10 TDVecEnv with masks
def test_vec_env_mask_describes_the_state_the_macro_step_left():
    L, B = 10, 64
    env = E.TDVecEnv(L, B, "def", seed=500, frame_skip=4, action_mask=True)
    try:
        assert env.frame_skip == 4 and env.engine.frame_skip == 4
        env.reset()
        mask = env.action_masks()["def"].cpu().numpy()
        rngs = [np.random.RandomState(1000 + b) for b in range(B)]
        acted = 0
        for i in range(20):
            picks = [M.pick_def(r, row, L * L) for r, row in zip(rngs, mask)]
            acts = np.asarray([M.def_action(p, L, False) for p in picks], dtype=np.int64)
            _, _, _, infos = env.step(torch.from_numpy(acts))
            assert np.array_equal(infos["RealAction"].cpu().numpy(), acts), i  # every sampled action was executed
            assert (infos["FailCode"].cpu().numpy() == 0).all(), i
            acted += sum(p >= 0 for p in picks)
            mask = infos["action_mask"].cpu().numpy()
        assert acted > B
        assert (env.engine.export_state()["hdr"]["steps"] % 4 == 0).all()
        assert (env.engine.flags() == 0).all()
    finally:
        env.close()


# ------------------------------------------------------------------ names, timing, single envs
@pytest.mark.parametrize("dtype,stem", [(torch.float32, "td_skip_kernel"), (torch.float16, "td_skip_kernel_f16")])
def test_kernel_name_kind_and_timing(dtype, stem):
    seeds = np.arange(8) + 500
    eng = TDEngine(20, 8, "2p", False, 1, np_seeds=seeds, py_seeds=seeds, obs_dtype=dtype, step_kernel="small")
    try:
        k1 = eng.step_kernel_name
        assert "td_step_kernel_small" in k1
        eng.set_frame_skip(4)
        assert eng.step_kernel_name == "%s<20, 2>" % stem
        assert "td_step_kernel_small" not in eng.step_kernel_name
        assert eng.step_kernel == "small"  # the k = 1 choice is kept
        eng.reset_all()
        eng.kernel_timing(3)
        for _ in range(3):
            _step(eng, _empty(eng))
        t = eng.kernel_times()
        assert len(t) == 3 and (t > 0).all()
        eng.set_frame_skip(1)
        assert eng.step_kernel_name == k1
    finally:
        eng.close()


def test_single_env_keyword():
    """TDDefense(..., frame_skip=4): one step() equals four steps of a twin (action, then empty)."""
    a = E.TDDefense(10, seed=503, opponent_seed=503, frame_skip=4)
    b = E.TDDefense(10, seed=503, opponent_seed=503)
    try:
        assert a.frame_skip == 4 and b.frame_skip == 1
        rng = np.random.RandomState(9)
        for i in range(10):
            act = int(rng.randint(0, 601))
            oa, ra, da, ia = a.step(act)
            tot = None
            for j in range(4):
                ob, rb, db, ib = b.step(act if j == 0 else b.empty_action())
                tot = rb if j == 0 else tot + rb
                if j == 0:
                    first = ib
                assert not db
            assert ra.hex() == tot.hex() and not da and np.array_equal(oa, ob), i
            assert ia["RealAction"] == first["RealAction"] and ia["FailCode"] == first["FailCode"], i
            assert ia["AllowNextMove"] == ib["AllowNextMove"] and ia["Win"] is None
    finally:
        a.close()
        b.close()
