"""The retained observation (td_retain_obs, TDEngine(retain_obs=True)) on the GPU.

A step into the retained buffer leaves unwritten the windows of a board's observation whose
dirty classes are all clean.  The buffer must still hold, byte for byte, what a full write
leaves -- so every test here steps a retained engine beside a twin built with
retain_obs=False (same seeds, same actions) and compares the observation bytes and every
other output after every step.

Episodes are 40 steps long (max_episode_steps), enemies cross a board side in 10-25 steps
and both sides are richer than the defaults, so that within 150 steps every board
auto-resets several times, towers are built / upgraded / destroyed, enemies appear, die or
leak, and bases lose life points; the twin run counts these events on the non-retained
engine and refuses a run without them.  Shapes: L = 10 with 33 boards (a board is 1,125 16-B units: 8 consecutive
boards start at all 8 unit offsets of a 128-B line, and 33 is odd), L = 20 TD-2p
multi-action and L = 30 with 9 boards."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import params as P  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402

EP, STEPS, SEED0 = 40, 150, 7300
OUTPUTS = ("obs", "reward", "done", "win", "allow_next", "cooldowns", "ep_return", "ep_len", "real_def", "fail_def",
           "real_atk", "fail_atk")


def _hp(multi):
    hp = P.HyperParameters()
    object.__setattr__(hp, "max_episode_steps", EP)
    object.__setattr__(hp, "allow_multiple_actions", bool(multi))
    return hp


def _cfg(L=10):
    c = copy.deepcopy(P.config)
    # a road is a few board sides long: enemies cross it well inside a 40-step episode
    c.enemy_speed = [[.1 * L] * 2, [.05 * L] * 2, [.04 * L] * 2, [.04 * L] * 2]
    c.attacker_init_cost = 30
    c.defender_init_cost = 30
    c.defender_cost_rate = 1.
    return c


def _engine(L, B, mode, multi, kernel, dtype, retain, autoreset=True, random_agent=True):
    seeds = SEED0 + np.arange(B)
    return TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=autoreset, cfg=_cfg(L), hp=_hp(multi),
                    step_kernel=kernel, obs_dtype=dtype, retain_obs=retain, random_agent=random_agent)


def _actions(rng, eng):
    L, n, d, a = eng.L, eng.B, None, None
    if eng.mode != "atk":
        d = (rng.random_sample((n, 6, L, L)) < 0.01).astype(np.int64) if eng.multi else \
            rng.randint(0, 6 * L * L + 1, size=n).astype(np.int64)
        d = torch.from_numpy(d).to(eng.device)
    if eng.mode != "def":
        a = torch.from_numpy(rng.randint(0, 5, size=(n, 3, 8)).astype(np.int64)).to(eng.device)
    return d, a


def _noop(eng):
    d = a = None
    if eng.mode != "atk":
        d = torch.zeros((eng.B, 6, eng.L, eng.L), dtype=torch.int64, device=eng.device) if eng.multi else \
            torch.full((eng.B,), 6 * eng.L * eng.L, dtype=torch.int64, device=eng.device)
    if eng.mode != "def":
        a = torch.full((eng.B, 3, 8), 4, dtype=torch.int64, device=eng.device)
    return d, a


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, where):
    """Every output of engine a equals engine b's, as bytes."""
    for name in OUTPUTS:
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), name
        if ta is None or torch.equal(_bytes(ta), _bytes(tb)):
            continue
        if name == "obs":
            diff = (_bytes(ta) != _bytes(tb)).reshape(a.B, 45, -1).any(dim=2).cpu().numpy()
            bd = np.flatnonzero(diff.any(axis=1))
            raise AssertionError(("observation bytes", where, "boards", bd[:8].tolist(), "channels of the first",
                                  np.flatnonzero(diff[bd[0]]).tolist()))
        raise AssertionError((name, where))


def _reset(eng, mask):
    """reset(mask), failing layout draws redrawn (as reset_all does for every board)."""
    m = np.asarray(mask, dtype=bool)
    for _ in range(64):
        failed = eng.reset(m)[1]
        if not failed:
            return
        m = np.zeros(eng.B, dtype=bool)
        m[failed] = True
    raise AssertionError("road generation kept failing")


def _snap(eng):
    st = eng.export_state()
    h = st["hdr"]
    return {"n_en": h["n_en"].copy(), "n_tw": h["n_tw"].copy(), "lp": h["base_LP"].copy(),
            "tw": (st["tw_inf"] & 0xFFFF).copy()}


class Events(object):
    def __init__(self):
        self.resets = self.towers = self.enemy_in = self.enemy_out = self.lp = 0

    def count(self, prev, cur, done):
        keep = ~done  # boards that kept their episode (the others were reset)
        self.resets += int(done.sum())
        tw = (prev["n_tw"] != cur["n_tw"]) | (prev["tw"] != cur["tw"]).any(axis=1)
        self.towers += int((tw & keep).sum())
        self.enemy_in += int(((prev["n_en"] == 0) & (cur["n_en"] > 0) & keep).sum())
        self.enemy_out += int(((prev["n_en"] > 0) & (cur["n_en"] == 0) & keep).sum())
        self.lp += int(((cur["lp"] < prev["lp"]) & keep).sum())

    def check(self, B):
        assert self.resets >= 2 * B, ("every board should restart several times", self.resets)
        assert self.towers > 0, "no step changed a tower list"
        assert self.enemy_in > 0 and self.enemy_out > 0, ("no board went from no enemy to some and back",
                                                          self.enemy_in, self.enemy_out)
        assert self.lp > 0, "no base lost life points"


def _twin(L, B, mode, multi, kernel, dtype, autoreset=True, random_agent=True, steps=STEPS):
    a = _engine(L, B, mode, multi, kernel, dtype, True, autoreset, random_agent)
    b = _engine(L, B, mode, multi, kernel, dtype, False, autoreset, random_agent)
    try:
        assert a.retain_obs and _lib.lib.td_retained_obs(a._h) == a.obs.data_ptr()
        assert not b.retain_obs and _lib.lib.td_retained_obs(b._h) is None
        assert a.step_kernel == b.step_kernel == kernel
        a.reset_all()
        b.reset_all()
        _same(a, b, "reset")
        ev, prev, rng = Events(), _snap(b), np.random.RandomState(11)
        for k in range(steps):
            d, at = _actions(rng, a)
            a.step(d, at)
            b.step(d, at)
            _same(a, b, k)
            done = b.done.cpu().numpy().astype(bool)
            cur = _snap(b)
            ev.count(prev, cur, done)
            if not autoreset and done.any():  # explicit resets, into the retained buffer
                _reset(a, done)
                _reset(b, done)
                _same(a, b, ("reset", k))
                cur = _snap(b)
            prev = cur
        ev.check(B)
        sa, sb = a.export_state(), b.export_state()
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), ("state", key)
        assert (a.flags() == 0).all() and (b.flags() == 0).all()
    finally:
        a.close()
        b.close()


SHAPES = [(10, 33, "def", False), (20, 9, "2p", True), (30, 9, "def", False)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("kernel", ["large", "small", "small2"])
@pytest.mark.parametrize("L,B,mode,multi", SHAPES, ids=["L10-def", "L20-2p-multi", "L30-def"])
def test_retained_engine_equals_its_twin(L, B, mode, multi, kernel, dtype):
    _twin(L, B, mode, multi, kernel, dtype)


def test_twin_with_the_reset_kernel_behind_the_step():
    """random_agent=False: the finished boards are reset by td_autoreset_kernel, after a step
    that may have skipped their windows."""
    _twin(10, 33, "def", False, "small2", torch.float32, random_agent=False)


def test_twin_without_autoreset():
    """autoreset=False: finished boards are reset explicitly, into the retained buffer."""
    _twin(10, 33, "def", False, "small2", torch.float32, autoreset=False)


# ------------------------------------------------------------------ the skip happens
STATIC = [0, 1, 2, 3, 6, 7, 8]  # layout planes away from the always-dirty channels' windows


@pytest.mark.parametrize("kernel", ["large", "small", "small2"])
def test_clean_static_windows_are_left_unwritten(kernel):
    """The promise broken on purpose: a marker written into the static planes survives a
    step of the retained engine and is overwritten by the twin's."""
    B = 9
    a = _engine(10, B, "def", False, kernel, torch.float32, True)
    b = _engine(10, B, "def", False, kernel, torch.float32, False)
    try:
        for e in (a, b):
            e.reset_all()
            for ch in STATIC:
                e.obs[:, ch, 3:7, :] = 7.0  # rows away from the channel boundaries
            e.step(*_noop(e))
        oa, ob = a.obs.cpu().numpy(), b.obs.cpu().numpy()
        assert (oa[:, STATIC, 3:7, :] == 7.0).all(), "the retained engine rewrote clean static windows"
        assert (ob[:, STATIC, 3:7, :] != 7.0).all(), "the twin left a marker"
        oa[:, STATIC, 3:7, :] = ob[:, STATIC, 3:7, :]
        assert np.array_equal(oa, ob)  # everything else as the twin
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------- invalidation
class Pair(object):
    """A retained engine and its twin, a few steps into their episodes."""

    def __init__(self, kernel="small2", warm=6, B=17):
        self.a = _engine(10, B, "def", False, kernel, torch.float32, True)
        self.b = _engine(10, B, "def", False, kernel, torch.float32, False)
        self.rng = np.random.RandomState(3)
        self.a.reset_all()
        self.b.reset_all()
        self.steps(warm, "warm-up")

    def steps(self, n, where):
        for k in range(n):
            d, at = _actions(self.rng, self.a)
            self.a.step(d, at)
            self.b.step(d, at)
            _same(self.a, self.b, (where, k))

    def both(self, fn):
        fn(self.a)
        fn(self.b)

    def close(self):
        self.a.close()
        self.b.close()


@pytest.fixture
def pair():
    p = Pair()
    yield p
    p.close()


def test_swapped_buffer_is_written_whole(pair):
    def swap(e):
        e.obs = torch.full((e.B, 45, 10, 10), float("nan"), device=e.device)
        _bytes(e.obs).fill_(0xA5)
        e._io.obs = e.obs.data_ptr()
    pair.both(swap)
    assert _lib.lib.td_retained_obs(pair.a._h) is None  # the freed block dropped its retention
    pair.steps(3, "swapped")


def test_masked_reset(pair):
    mask = np.arange(pair.a.B) % 3 == 0
    pair.both(lambda e: e.reset(mask))
    _same(pair.a, pair.b, "reset(mask)")
    pair.steps(3, "after reset(mask)")


def test_reset_without_an_observation(pair):
    def reset_null(e):
        torch.cuda.synchronize(e.device)
        assert _lib.lib.td_reset(e._h, None, None, e._stream()) == 0
    pair.both(reset_null)
    pair.steps(3, "after td_reset(NULL obs)")


def test_set_config(pair):
    cfg = _cfg()
    cfg.tower_cost = [[14, 14], [17, 17], [23, 23], [12, 12]]
    cfg.max_cost = 80
    pair.both(lambda e: e.set_config(cfg, _hp(False)))
    pair.steps(3, "after td_set_config")


def test_obs_dtype_there_and_back(pair):
    pair.both(lambda e: e.set_obs_dtype(torch.float16))
    assert _lib.lib.td_retained_obs(pair.a._h) == pair.a.obs.data_ptr()
    pair.steps(2, "float16")
    pair.both(lambda e: e.set_obs_dtype(torch.float32))
    assert _lib.lib.td_retained_obs(pair.a._h) == pair.a.obs.data_ptr()
    pair.steps(3, "float32 again")


def test_import_state(pair):
    def move(e):
        st = e.export_state(1, 1)
        e.import_state(st, 0)  # board 0 becomes board 1: another layout, other towers and enemies
    pair.both(move)
    pair.steps(3, "after td_import_state")


def test_opponent_between_steps(pair):
    pair.both(lambda e: e.opponent("enemy", 1))
    pair.steps(3, "after td_opponent")


def test_freed_block_drops_its_retention(pair):
    lib, a = _lib.lib, pair.a
    nbytes = a.obs.numel() * 4

    def block():
        p = ctypes.c_void_p()
        assert lib.td_alloc_device(nbytes, a.device.index or 0, 0, ctypes.byref(p)) == 0 and p.value
        return p.value

    keep = a.obs  # (the engine's own block stays alive)
    p = block()
    try:
        assert lib.td_retain_obs(a._h, p) == 0 and lib.td_retained_obs(a._h) == p
        a._io.obs = p
        for k in range(3):
            d, at = _actions(pair.rng, a)
            a.step(d, at)
            pair.b.step(d, at)
        torch.cuda.synchronize(a.device)
        assert lib.td_free_device(p) == 0
        p = None
        assert lib.td_retained_obs(a._h) is None
        p = block()  # zeroed, possibly at the old address: never taken for the old buffer
        assert lib.td_retain_obs(a._h, p) == 0
        a._io.obs = p
        for k in range(3):
            d, at = _actions(pair.rng, a)
            a.step(d, at)
            pair.b.step(d, at)
            got = _read_block(p, keep)
            assert torch.equal(_bytes(got), _bytes(pair.b.obs)), ("new block", k)
    finally:
        torch.cuda.synchronize(a.device)
        lib.td_retain_obs(a._h, None)
        a._io.obs = keep.data_ptr()
        if p:
            lib.td_free_device(p)


def _read_block(ptr, like):
    """The bytes at device address ptr as a tensor shaped like ``like`` (a copy)."""
    class Raw(object):
        pass
    raw = Raw()
    raw.__cuda_array_interface__ = {"shape": tuple(like.shape), "typestr": "<f4", "data": (int(ptr), False),
                                    "version": 2, "strides": None}
    return torch.as_tensor(raw, device=like.device).clone()


def test_handle_that_never_retains_writes_every_byte():
    a = _engine(10, 33, "def", False, "small2", torch.float32, False)
    b = _engine(10, 33, "def", False, "small2", torch.float32, False)
    try:
        assert _lib.lib.td_retained_obs(a._h) is None
        a.reset_all()
        b.reset_all()
        rng = np.random.RandomState(5)
        for k in range(12):
            _bytes(a.obs).fill_(0xA5)
            d, at = _actions(rng, a)
            a.step(d, at)
            b.step(d, at)
            _same(a, b, k)
    finally:
        a.close()
        b.close()
