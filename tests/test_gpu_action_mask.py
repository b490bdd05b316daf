"""Legal-action masks computed on the device (td_action_mask / TDEngine.action_mask).

* the kernel equals gym_TD.masks.reference_masks (itself pinned to brute force on the CPU
  oracle, tests/test_action_mask_ref.py) for every board and every action, along runs
  whose policy samples from the kernel's masks only, across episode ends;
* the step is the judge: every action the policy chose was executed, and one exported
  state replicated over 6 L^2 + 1 boards shows mask[a] == "the step executed a" for every a;
* pitch, alignment, refusals, no side effect on the step, and the Python surface.

An attacker summon counts as executed when its road's fail code is 0 and the first slot of
RealAction kept its type (RealAction echoes the input while the cool-down blocks or the
road does not exist, as in the reference; fail_atk is -1 there)."""
import ctypes

import numpy as np
import pytest
import torch

import maskutil as M
from oracle import policies

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import envs as E  # noqa: E402
from gym_TD import vector as V  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402
from gym_TD.masks import reference_masks  # noqa: E402

FLAG_EN_OVERFLOW, FLAG_TW_OVERFLOW = 1, 2


def _engine(L, B, mode, multi, cfg, hp, autoreset, seed0=500):
    seeds = np.arange(B) + seed0
    if L == 7:  # no 7x7 map can be drawn: caller layouts, and the test restarts finished boards
        eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False, cfg=cfg, hp=hp)
        _restart_7(eng, np.arange(B))
        return eng
    eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=autoreset, cfg=cfg, hp=hp)
    eng.reset_all()
    return eng


def _restart_7(eng, boards):
    recs = M.hand_layouts_7()
    if len(boards):
        eng.reset_layouts(np.stack([recs[b % 2] for b in boards]), boards)


def _host(masks):
    return {k: v.cpu().numpy() for k, v in masks.items()}


def _choose(rngs, m, L, mode, multi):
    """One mask-legal action per board: (def picks, def actions, atk picks, atk actions)."""
    dk = da = ak = aa = None
    if mode != "atk":
        dk = [M.pick_def(r, row, L * L) for r, row in zip(rngs, m["def"])]
        da = np.stack([np.asarray(M.def_action(k, L, multi), dtype=np.int64) for k in dk])
    if mode != "def":
        ak = [M.pick_atk(r, row) for r, row in zip(rngs, m["atk"])]
        aa = np.stack([M.atk_action(rt) for rt in ak])
    return dk, da, ak, aa


def _step(eng, da, aa):
    eng.step(def_act=None if da is None else torch.from_numpy(da), atk_act=None if aa is None else torch.from_numpy(aa))


def _assert_equals_reference(eng, m, cfg, hp, where):
    st = eng.export_state()
    for b in range(eng.B):
        dm, dc, am = reference_masks(eng.board_state(b, st), eng.L, cfg, hp, eng.mode, eng.multi)
        if eng.mode != "atk":
            assert np.array_equal(m["def"][b], dm), (where, b, "def")
            assert np.array_equal(m["def_code"][b], dc), (where, b, "def_code")
        if eng.mode != "def":
            assert np.array_equal(m["atk"][b], am), (where, b, "atk")


# ------------------------------------------------- 1 + 2: the reference, and the step as judge
@pytest.mark.parametrize("mode,multi,L,B", [
    ("def", False, 10, 256), ("def", True, 10, 64), ("atk", False, 10, 64), ("2p", False, 20, 32),
    ("2p", True, 20, 32), ("def", False, 30, 16), ("def", False, 7, 32), ("def", False, 32, 8)])
def test_kernel_equals_reference_and_step_executes(mode, multi, L, B):
    """120 steps of the mask policy, auto-reset on, episodes of 60 steps; the kernel's masks and
    codes against the numpy reference for every board at every 10th step, every chosen action
    against the step's RealAction / FailCode.  (L = 7, the generic-L kernel with an odd cell
    count: create_road_v2 cannot draw a 7x7 map, so those boards start from caller layouts
    and the test restarts the finished ones itself.)"""
    cfg = M.config(M.RICH) if mode == "def" else M.config(M.RICH, M.ATK)
    hp = M.hyper(multi, max_episode_steps=60)  # episode ends and the next episode's masks inside the run
    eng = _engine(L, B, mode, multi, cfg, hp, autoreset=True)
    try:
        rngs = [np.random.RandomState(1000 + s) for s in range(B)]
        acted = {"def": 0, "atk": 0, "ops": np.zeros(6, dtype=int), "done": 0}
        A = 6 * L * L
        for k in range(120):
            check = k % 10 == 0
            m = _host(eng.action_mask(code=check))
            if check:
                _assert_equals_reference(eng, m, cfg, hp, k)
            dk, da, ak, aa = _choose(rngs, m, L, mode, multi)
            _step(eng, da, aa)
            acted["done"] += int(eng.done.sum().item())
            if L == 7:
                _restart_7(eng, np.flatnonzero(eng.done.cpu().numpy()))
            if mode != "atk":
                rd = eng.real_def.cpu().numpy()
                if multi:
                    assert np.array_equal(rd, da), k  # the one flag set, and nothing else
                else:
                    assert np.array_equal(rd, da), k
                    assert (eng.fail_def.cpu().numpy() == 0).all(), k
                for a in dk:
                    if a >= 0:
                        acted["def"] += 1
                        acted["ops"][a // (L * L)] += 1
                assert all(a < A for a in dk)
            if mode == "atk":
                ra, fa = eng.real_atk.cpu().numpy(), eng.fail_atk.cpu().numpy()
                for b, rt in enumerate(ak):
                    if rt is not None:
                        assert ra[b, rt[0], 0] == rt[1] and fa[b, rt[0]] == 0, (k, b, rt)
                        acted["atk"] += 1
        assert (eng.flags() == 0).all()
        assert acted["done"] > 0  # masks of fresh episodes were compared
        assert mode == "atk" or (acted["def"] > 0 and (acted["ops"][:4].sum() > 0))
        assert mode != "atk" or acted["atk"] > 0
    finally:
        eng.close()


# ------------------------------------------------------------- 3: exhaustive truth on one state
def _replicate(st, n):
    return {k: np.repeat(v[:1], n, axis=0) for k, v in st.items()}


def _find_state(eng, cfg, hp, want, steps, mode="def"):
    """Play the mask policy until some board's state satisfies want(header, board_state);
    returns that board's exported state (count 1)."""
    rngs = [np.random.RandomState(1000 + s) for s in range(eng.B)]
    for _ in range(steps):
        st = eng.export_state()
        for b in range(eng.B):
            if want(st["hdr"][b], eng.board_state(b, st)):
                return {k: v[b:b + 1].copy() for k, v in st.items()}
        m = _host(eng.action_mask())
        _, da, _, aa = _choose(rngs, m, eng.L, mode, False)
        _step(eng, da, aa)
    raise AssertionError("no board reached the wanted state in %d steps" % steps)


def _def_sources():
    L, hp = 10, M.hyper()
    out = {}
    cfg = M.config(M.RICH)
    eng = _engine(L, 16, "def", False, cfg, hp, autoreset=False)
    try:
        def both_levels(h, s):
            lv = {t[1] for t in s["towers"]}
            return h["def_cd"] <= 1 and lv == {0, 1} and 12 <= s["cost_def"] < 23  # type 2 (23) is too dear
        out["rich"] = (cfg, _find_state(eng, cfg, hp, both_levels, 200))
        out["blocked"] = (cfg, _find_state(eng, cfg, hp, lambda h, s: h["def_cd"] > 1 and len(s["towers"]) > 0, 200))
    finally:
        eng.close()
    cfg = M.config(M.CAP)
    eng = _engine(L, 4, "def", False, cfg, hp, autoreset=False)
    try:
        out["cap"] = (cfg, _find_state(eng, cfg, hp, lambda h, s: h["n_tw"] == 32 and h["def_cd"] <= 1, 300))
    finally:
        eng.close()
    return out


@pytest.fixture(scope="module")
def def_sources():
    return _def_sources()


@pytest.mark.parametrize("which", ["rich", "blocked", "cap"])
def test_exhaustive_defender_truth(def_sources, which):
    L, hp = 10, M.hyper()
    A = 6 * L * L + 1
    cfg, src = def_sources[which]
    eng = TDEngine(L, A, "def", False, 1, autoreset=False, cfg=cfg, hp=hp)
    try:
        eng.import_state(_replicate(src, A))
        m = _host(eng.action_mask(code=True))
        assert (m["def"] == m["def"][0]).all() and (m["def_code"] == m["def_code"][0]).all()
        mask, code = m["def"][0], m["def_code"][0]
        dm, dc, _ = reference_masks(eng.board_state(0), L, cfg, hp, "def", False)
        assert np.array_equal(mask, dm) and np.array_equal(code, dc)
        act = np.arange(A, dtype=np.int64)
        _step(eng, act, None)
        real, fail = eng.real_def.cpu().numpy(), eng.fail_def.cpu().numpy()
        assert np.array_equal(mask != 0, real == act)
        actionable = int(src["hdr"][0]["def_cd"]) <= 1
        assert actionable == (which != "blocked")
        if actionable:
            assert np.array_equal(code, fail)
        flags = eng.flags()
        if which == "rich":
            assert {0, 1, 2, 3, 4} <= set(code.tolist()) and mask[:-1].any() and not mask[:-1].all()
            assert (flags == 0).all()
        elif which == "blocked":
            assert mask[-1] == 1 and not mask[:-1].any() and code[:-1].any()
            assert (flags == 0).all()
        else:
            free = np.asarray(eng.board_state(0)["map6"]) == 0  # (board 0 took action 0: a refused build)
            builds = code[:4 * L * L].reshape(4, L * L)
            assert free.any() and (builds[:, free] == 6).all() and (builds[:, ~free] == 2).all()
            assert not mask[:4 * L * L].any()
            want = np.zeros(A, dtype=np.int32)
            want[:4 * L * L] = np.where(np.tile(free, 4), FLAG_TW_OVERFLOW, 0)
            assert np.array_equal(flags, want)
    finally:
        eng.close()


def _atk_executed(eng):
    ra, fa = eng.real_atk.cpu().numpy(), eng.fail_atk.cpu().numpy()
    return np.array([fa[b, b // 4] == 0 and ra[b, b // 4, 0] == b % 4 for b in range(12)])


@pytest.mark.parametrize("which", ["mixed", "blocked", "crowd"])
def test_exhaustive_attacker_truth(which):
    """12 replicated TD-atk boards, one (road, type) each."""
    L, hp = 10, M.hyper()
    if which == "crowd":  # 128 live enemies: nothing can be summoned
        cfg = M.config(M.CROWD)
        src_eng = _engine(L, 2, "atk", False, cfg, hp, autoreset=False)
        try:
            full = np.zeros((2, 3, 8), dtype=np.int64)
            for _ in range(40):
                st = src_eng.export_state()
                if (st["hdr"]["n_en"] == 128).any():
                    break
                _step(src_eng, None, full)
            b = int(np.argmax(st["hdr"]["n_en"] == 128))
            assert st["hdr"]["n_en"][b] == 128 and st["hdr"]["atk_cd"][b] <= 1 and st["hdr"]["cost_atk"][b] >= 1
            src = {k: v[b:b + 1].copy() for k, v in st.items()}
        finally:
            src_eng.close()
    else:
        cfg = M.config(M.ATK)
        src_eng = _engine(L, 16, "atk", False, cfg, hp, autoreset=False)
        try:
            if which == "mixed":  # a missing road, and money for some types only
                def want(h, s):
                    return h["atk_cd"] <= 1 and h["num_roads"] < 3 and 8 <= s["cost_atk"] < 30
            else:
                def want(h, s):
                    return h["atk_cd"] > 1 and s["cost_atk"] >= 8
            src = _find_state(src_eng, cfg, hp, want, 200, mode="atk")
        finally:
            src_eng.close()
    eng = TDEngine(L, 12, "atk", False, 1, autoreset=False, cfg=cfg, hp=hp)
    try:
        eng.import_state(_replicate(src, 12))
        for f in src["hdr"]["flags"]:
            assert f in (0, FLAG_EN_OVERFLOW)
        m = _host(eng.action_mask())["atk"]
        assert (m == m[0]).all() and (m[0][:, 4] == 1).all()
        _, _, am = reference_masks(eng.board_state(0), L, cfg, hp, "atk", False)
        assert np.array_equal(m[0], am)
        act = np.stack([M.atk_action((b // 4, b % 4)) for b in range(12)])
        _step(eng, None, act)
        assert np.array_equal(m[0][:, :4].reshape(12) != 0, _atk_executed(eng))
        if which == "mixed":
            assert m[0][:, :4].any() and not m[0][0, :4].all() and not m[0][2, :4].any()
        else:
            assert not m[0][:, :4].any()
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 4: pitch
def _raw_mask(eng, def_mask=None, def_code=None, atk_mask=None, pitch=0, size=None):
    io = _lib.TdMaskIO(def_mask=def_mask, def_code=def_code, atk_mask=atk_mask, def_pitch=pitch)
    if size is not None:
        io.size = size
    rc = _lib.lib.td_action_mask(eng._h, io, eng._stream())
    err = _lib.lib.td_last_error().decode() if rc < 0 else ""
    torch.cuda.synchronize()
    return rc, err


@pytest.fixture(scope="module")
def played():
    """A 33-board discrete TD-def engine 40 mask-policy steps into the rich config."""
    cfg, hp = M.config(M.RICH), M.hyper()
    eng = _engine(10, 33, "def", False, cfg, hp, autoreset=True)
    rngs = [np.random.RandomState(1000 + s) for s in range(eng.B)]
    for _ in range(40):
        _, da, _, _ = _choose(rngs, _host(eng.action_mask()), 10, "def", False)
        _step(eng, da, None)
    yield eng
    eng.close()


@pytest.mark.parametrize("pitch,off_mask,off_code", [
    (601, 0, 0), (608, 0, 0), (0, 0, 0), (640, 0, 0), (601, 1, 1), (608, 1, 1), (608, 5, 0), (601, 0, None)])
def test_pitch_and_alignment_give_the_same_bytes(played, pitch, off_mask, off_code):
    eng, A, GUARD = played, 601, 64
    m = _host(eng.action_mask(code=True))
    want_m, want_c = m["def"].copy(), m["def_code"].copy()
    assert want_m.shape == (eng.B, A) and want_m[:, :-1].any() and want_c.any()
    p = pitch or A
    n = eng.B * p

    def buf(off):
        t = torch.full((16 + off + n + GUARD,), 0xAA, dtype=torch.uint8, device=eng.device)
        assert t.data_ptr() % 16 == 0
        return t, t.data_ptr() + 16 + off

    tm, pm = buf(off_mask)
    tc, pc = buf(off_code) if off_code is not None else (None, None)
    rc, err = _raw_mask(eng, def_mask=pm, def_code=pc, pitch=pitch)
    assert rc == 0, err
    for t, off, want in ((tm, off_mask, want_m), (tc, off_code, want_c)):
        if t is None:
            continue
        h = t.cpu().numpy()
        assert (h[:16 + off] == 0xAA).all() and (h[16 + off + n:] == 0xAA).all()  # nothing outside B * pitch
        rows = h[16 + off:16 + off + n].reshape(eng.B, p)
        assert np.array_equal(rows[:, :A], want)
        assert (rows[:, A:] == 0).all()  # padding inside the pitch


def test_multi_action_rows_at_every_alignment():
    """[B][6][L][L] rows of 600 / 294 bytes start at every other 8-byte / 2-byte phase."""
    for L in (10, 7):
        cfg, hp = M.config(M.RICH), M.hyper(True)
        eng = _engine(L, 9, "def", True, cfg, hp, autoreset=True)
        try:
            rngs = [np.random.RandomState(1000 + s) for s in range(eng.B)]
            for _ in range(20):  # (episodes last 1,200 steps: no board finishes here)
                _, da, _, _ = _choose(rngs, _host(eng.action_mask()), L, "def", True)
                _step(eng, da, None)
            want = _host(eng.action_mask(code=True))
            n = eng.B * 6 * L * L
            for off in (0, 3):
                t = torch.full((16 + off + n + 64,), 0xAA, dtype=torch.uint8, device=eng.device)
                rc, err = _raw_mask(eng, def_code=t.data_ptr() + 16 + off)
                assert rc == 0, err
                h = t.cpu().numpy()
                assert (h[:16 + off] == 0xAA).all() and (h[16 + off + n:] == 0xAA).all()
                assert np.array_equal(h[16 + off:16 + off + n].reshape(eng.B, 6, L, L), want["def_code"])
        finally:
            eng.close()


# ----------------------------------------------------------------------- 5: no side effect
def test_masks_do_not_change_the_step():
    cfg, hp = M.config(M.RICH), M.hyper(max_episode_steps=30)
    a = _engine(10, 64, "def", False, cfg, hp, autoreset=True)
    b = _engine(10, 64, "def", False, cfg, hp, autoreset=True)
    try:
        rng = np.random.RandomState(7)
        for k in range(50):
            act = np.array([policies.discrete_def(rng, 10) for _ in range(64)], dtype=np.int64)
            _step(a, act, None)
            _step(b, act, None)
            b.action_mask(code=True)
            assert np.array_equal(a.obs.cpu().numpy().view(np.uint32), b.obs.cpu().numpy().view(np.uint32)), k
            assert np.array_equal(a.reward.cpu().numpy().view(np.uint64), b.reward.cpu().numpy().view(np.uint64)), k
            assert np.array_equal(a.done.cpu().numpy(), b.done.cpu().numpy()), k
        sa, sb = a.export_state(), b.export_state()
        for name in sa:
            assert np.array_equal(sa[name], sb[name]), name
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------ 6: refusals
def test_refusals_launch_nothing(played):
    eng = played
    t = torch.full((eng.B * 608 + 64,), 0xAA, dtype=torch.uint8, device=eng.device)
    p = t.data_ptr()
    cases = {
        "size": dict(def_mask=p, size=ctypes.sizeof(_lib.TdMaskIO) - 8),
        "all NULL": dict(),
        "atk": dict(atk_mask=p),
        "pitch": dict(def_mask=p, pitch=600),
    }
    for name, kw in cases.items():
        rc, err = _raw_mask(eng, **kw)
        assert rc < 0 and name.split()[0] in err, (name, rc, err)
        assert (t.cpu().numpy() == 0xAA).all(), name
    cfg, hp = M.config(M.RICH), M.hyper(True)
    multi = _engine(10, 4, "def", True, cfg, hp, autoreset=True)
    atk = _engine(10, 4, "atk", False, M.config(M.ATK), M.hyper(), autoreset=True)
    try:
        rc, err = _raw_mask(multi, def_mask=p, pitch=608)
        assert rc < 0 and "pitch" in err, err
        rc, err = _raw_mask(atk, def_code=p)
        assert rc < 0 and "defender" in err, err
        assert (t.cpu().numpy() == 0xAA).all()
    finally:
        multi.close()
        atk.close()


# ----------------------------------------------------------------------- 7: Python surface
def test_vec_env_infos_and_vector_env():
    plain = E.TDVecEnv(10, 8, "def", seed=3)
    masked = E.TDVecEnv(10, 8, "def", seed=3, action_mask=True)
    two = E.TDVecEnv(10, 8, "2p", seed=3, action_mask=True)
    try:
        for v in (plain, masked, two):
            v.reset()
        act = torch.full((8,), 600, dtype=torch.int64)
        _, _, _, inf = plain.step(act)
        assert "action_mask" not in inf and "action_mask_attacker" not in inf
        _, _, _, inf = masked.step(act)
        m = inf["action_mask"]
        assert m.dtype == torch.uint8 and tuple(m.shape) == (8, 601) and "action_mask_attacker" not in inf
        assert torch.equal(m, masked.engine.action_mask()["def"]) and bool((m[:, -1] == 1).all())
        assert torch.equal(masked.action_masks()["def"], m)
        _, _, _, inf = two.step({"Defender": act, "Attacker": torch.full((8, 3, 8), 4, dtype=torch.int64)})
        assert tuple(inf["action_mask"].shape) == (8, 601) and tuple(inf["action_mask_attacker"].shape) == (8, 3, 5)
    finally:
        for v in (plain, masked, two):
            v.close()
    ve = V.VectorEnv("TD-def-small-v0", 4, seed=11)
    try:
        ve.reset()
        ve.step(np.full(4, 600))
        m = ve.action_masks()
        assert set(m) == {"def"} and isinstance(m["def"], np.ndarray)
        assert m["def"].dtype == np.uint8 and m["def"].shape == (4, 601)
        assert np.array_equal(m["def"], ve.vec.engine.action_mask()["def"].cpu().numpy())
    finally:
        ve.close()
    env = E.TDAttack(10, seed=2, opponent_seed=2)
    try:
        m = env.action_mask()
        assert m.dtype == np.uint8 and m.shape == (3, 5) and (m[:, 4] == 1).all()
    finally:
        env.close()
