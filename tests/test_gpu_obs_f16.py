"""The float16 observation (td_set_obs_format, TDEngine(obs_dtype=torch.float16)) on the GPU.

Each float16 value must be the float32 value the engine writes by default, rounded to
nearest-even.  The oracle is the batched C restatement (oracle.td_cpu.Batch): its float32
observation converted with numpy's astype(np.float16), which rounds to nearest-even, and
compared as bytes -- no tolerance.  A packed convert that rounds toward zero differs from it
in the inexact ratios (life points, costs, progress) of every step.

Shapes: 40 boards with 1-LP bases (short episodes: the auto-reset's observation is compared
too), seeds 4100 + i, actions from RandomState(5).  A board is 9,000 B at L = 10 and 81,000 B
at L = 30 -- multiples of 8 B, not of 16 B or of the 128-B line -- so 40 consecutive boards
start at all 16 unit offsets of a line and at both 8-B parities, and both ends of the batch
border memory that is no board.  On the oracle (CPU), boards that finish an episode / the
first step one does:
    L = 10 def, 96 steps: 5 / 44        L = 20 2p multi-action, 160 steps: 26 / 76
    L = 30 def, 200 steps: 21 / 108     L = 12 2p discrete, 96 steps: 8
    L = 11 def, 64 steps: 4             L = 9 atk, 64 steps: 1
    L = 32 def, 160 steps: 10 / 119     L = 31 atk, 160 steps: 3 / 135
At L = 31 / 32 an enemy needs over a hundred steps to walk a road, so no board finishes within
48 steps (measured: 0 of 40 at both sizes); those two shapes run 160 steps -- their first 48 are
the 48-step run -- so that the auto-reset's observation is compared there too.
"""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import params as P  # noqa: E402
from gym_TD import vector  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402
from gym_TD.envs import TDVecEnv  # noqa: E402
from oracle import td_cpu as C  # noqa: E402
from oracle import td_oracle as O  # noqa: E402

B, SEED0 = 40, 4100


def _cfgs():
    dcfg = copy.deepcopy(P.config)
    dcfg.base_LP = 1
    return O.Config(base_LP=1), dcfg


def _actions(rng, L, mode, multi, n):
    d = a = None
    if mode != "atk":
        d = (rng.random_sample((n, 6, L, L)) < 0.01).astype(np.int64) if multi else \
            rng.randint(0, 6 * L * L + 1, size=n).astype(np.int64)
    if mode != "def":
        a = rng.randint(0, 5, size=(n, 3, 8)).astype(np.int64)
    return d, a


@functools.lru_cache(maxsize=1)  # one trajectory at a time: the kernels of a shape run back to back
def _oracle(L, mode, multi, steps):
    """The oracle's trajectory, computed once per shape: the first observation and, per step,
    (defender actions, attacker actions, float16 observation, reward, done)."""
    ocfg, _ = _cfgs()
    seeds = SEED0 + np.arange(B)
    bt = C.Batch(L, B, mode, 1, seeds, seeds, cfg=ocfg, multi=multi)
    try:
        assert bt.initial_failed == []
        first = bt.obs().astype(np.float16)
        rng = np.random.RandomState(5)
        o32 = np.empty((B, 45, L, L), dtype=np.float32)
        traj = []
        for _ in range(steps):
            d, a = _actions(rng, L, mode, multi, B)
            rw, dn = bt.step(d, a, obs=o32)
            assert np.isfinite(o32).all() and float(np.abs(o32).max()) < 65504.0  # no float16 overflow
            traj.append((d, a, o32.astype(np.float16), rw.copy(), dn.copy()))
        assert not bt.no_layout().any()
    finally:
        bt.close()
    for t in [first] + [s[2] for s in traj]:
        t.setflags(write=False)
    return first, traj


def _run(L, mode, multi, steps, kernel):
    first, traj = _oracle(L, mode, multi, steps)
    _, dcfg = _cfgs()
    seeds = SEED0 + np.arange(B)
    eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, cfg=dcfg,
                   step_kernel=kernel, obs_dtype=torch.float16)
    try:
        assert eng.obs.dtype == torch.float16 and eng.obs_dtype == torch.float16
        assert "_f16<" in eng.step_kernel_name, eng.step_kernel_name
        if kernel != "auto":
            assert eng.step_kernel == kernel
        obs, _ = eng.reset_all()
        assert np.array_equal(obs.cpu().numpy().view(np.uint16), first.view(np.uint16)), "first observation"
        finished = np.zeros(B, dtype=bool)
        enemy_steps = 0
        for k, (d, a, want, rw_c, dn_c) in enumerate(traj):
            eng.step(def_act=None if d is None else torch.from_numpy(d).to(eng.device),
                     atk_act=None if a is None else torch.from_numpy(a).to(eng.device))
            rw, dn = eng.reward.cpu().numpy(), eng.done.cpu().numpy()
            bad = np.flatnonzero(rw.view(np.uint64) != rw_c.view(np.uint64))
            assert bad.size == 0, ("reward bits", k, bad[:8].tolist())
            assert np.array_equal(dn, dn_c), ("done", k)
            got = eng.obs.cpu().numpy()
            if not np.array_equal(got.view(np.uint16), want.view(np.uint16)):
                diff = (got.view(np.uint16) != want.view(np.uint16))
                b = int(np.flatnonzero(diff.reshape(B, -1).any(axis=1))[0])
                ch, r, c = [int(v[0]) for v in np.nonzero(diff[b])]
                raise AssertionError(("observation bytes", k, b, ch, r, c, float(got[b, ch, r, c]),
                                      float(want[b, ch, r, c]), int(diff.sum())))
            finished |= dn.astype(bool)
            enemy_steps += int(want[:, 25:41].any())
        assert finished.any(), "no board finished: the auto-reset's observation was not compared"
        assert enemy_steps > 0, "no enemy on any board: channels 25-40 were never non-zero"
        assert (eng.flags() == 0).all(), np.unique(eng.flags(), return_counts=True)
    finally:
        eng.close()


# the shapes with the line writer (write_obs_lines), on each of the three step kernels
@pytest.mark.parametrize("L,mode,multi,steps,kernel", [
    (L, mode, multi, steps, kernel)
    for L, mode, multi, steps in [(10, "def", False, 96), (20, "2p", True, 160), (30, "def", False, 200)]
    for kernel in ("large", "small", "small2")])
def test_f16_obs_is_rounded_f32_obs(L, mode, multi, steps, kernel):
    _run(L, mode, multi, steps, kernel)


# generic L: the quad path (L^2 % 4 == 0, 8-B-aligned boards) and the per-element path
# and the ends of the size range: 32 (quad path, NC = 1024) and 31 (per-element path, NC = 961)
@pytest.mark.parametrize("L,mode,steps", [(12, "2p", 96), (11, "def", 64), (9, "atk", 64), (32, "def", 160),
                                          (31, "atk", 160)])
def test_f16_obs_generic_map_size(L, mode, steps):
    _run(L, mode, False, steps, "auto")


def _run_into(buf, off, nbytes, L, n, steps):
    """n boards stepped with the observation at byte `off` of `buf`; returns the board bytes."""
    seeds = 900 + np.arange(n)
    eng = TDEngine(L, n, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, obs_dtype=torch.float16)
    try:
        eng.obs = buf[off:off + nbytes].view(torch.float16).view(n, 45, L, L)
        eng._io.obs = eng.obs.data_ptr()
        assert eng.obs.data_ptr() == buf.data_ptr() + off
        eng.reset_all()
        out = [buf[off:off + nbytes].clone()]
        g = torch.Generator(device="cuda").manual_seed(3)
        for _ in range(steps):
            eng.step(def_act=torch.randint(0, 6 * L * L + 1, (n,), device="cuda", generator=g, dtype=torch.int64))
            out.append(buf[off:off + nbytes].clone())
        torch.cuda.synchronize()
        assert (eng.flags() == 0).all()
    finally:
        eng.close()
    return out


def test_f16_obs_stays_inside_its_buffer():
    """The observation at +0, +8 (the other 8-B parity: line writer) and +2 bytes (per-element
    path) into a larger buffer of 0xA5: the same board bytes, and not a byte outside them."""
    L, n, steps, pad = 10, 33, 8, 1024
    nbytes = n * 45 * L * L * 2
    ref = None
    for shift in (0, 8, 2):
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 128 == 0
        out = _run_into(buf, pad + shift, nbytes, L, n, steps)
        guard = torch.cat([buf[:pad + shift], buf[pad + shift + nbytes:]])
        assert bool((guard == 0xA5).all()), ("bytes outside the boards were written", shift)
        if ref is None:
            ref = out
            assert not bool((ref[-1] == 0xA5).all())
        else:
            for k, (x, y) in enumerate(zip(out, ref)):
                assert torch.equal(x, y), ("board bytes differ from the run at offset 0", shift, k)


def test_format_switch_disturbs_no_state():
    L, n = 10, 64
    seeds = 300 + np.arange(n)
    a = TDEngine(L, n, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True)
    b = TDEngine(L, n, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True)
    try:
        a.reset_all()
        b.reset_all()
        g = torch.Generator(device="cuda").manual_seed(11)
        f32 = a.obs

        def steps(k):
            for _ in range(k):
                d = torch.randint(0, 6 * L * L + 1, (n,), device="cuda", generator=g, dtype=torch.int64)
                a.step(def_act=d)
                b.step(def_act=d)
                if a.obs.dtype == torch.float32:
                    assert torch.equal(a.obs, b.obs)
                else:  # torch's conversion rounds to nearest-even too
                    assert torch.equal(a.obs.view(torch.int16), b.obs.half().view(torch.int16))
                assert torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done)

        steps(12)
        name32 = a.step_kernel_name
        a.set_obs_dtype(torch.float16)
        assert a.obs.dtype == torch.float16 and _lib.lib.td_obs_format(a._h) == _lib.OBS_F16
        assert a.step_kernel_name == name32.replace("<", "_f16<", 1)
        steps(12)
        a.set_obs_dtype(torch.float32, f32)
        assert a.step_kernel_name == name32 and a.step_kernel_name == b.step_kernel_name
        steps(12)
        assert (a.flags() == 0).all() and (b.flags() == 0).all()
    finally:
        a.close()
        b.close()


def test_obs_format_calls():
    L, n = 10, 16
    eng = TDEngine(L, n, "def", False, 1, np_seeds=np.arange(n), py_seeds=np.arange(n))
    try:
        lib, h = _lib.lib, eng._h
        assert lib.td_obs_format(h) == _lib.OBS_F32 and lib.td_obs_bytes(h) == n * 45 * L * L * 4
        assert lib.td_set_obs_format(h, 7) < 0 and b"format" in lib.td_last_error()
        assert lib.td_obs_format(h) == _lib.OBS_F32 and lib.td_obs_bytes(h) == n * 45 * L * L * 4
        assert lib.td_set_obs_format(h, _lib.OBS_F16) == 0
        assert lib.td_obs_format(h) == _lib.OBS_F16 and lib.td_obs_bytes(h) == n * 45 * L * L * 2
        assert lib.td_set_obs_format(h, -1) < 0 and lib.td_obs_format(h) == _lib.OBS_F16
        assert lib.td_set_obs_format(h, _lib.OBS_F32) == 0 and lib.td_obs_format(h) == _lib.OBS_F32
        assert lib.td_abi_version() == 3 and lib.td_step_io_size() == 120
    finally:
        eng.close()


def test_vec_env_f16_with_action_masks():
    L, n = 10, 48
    h = TDVecEnv(L, n, "def", seed=70, action_mask=True, obs_dtype=torch.float16)
    f = TDVecEnv(L, n, "def", seed=70, action_mask=True)
    try:
        assert h.observation_space.dtype == np.float16 and f.observation_space.dtype == np.float32
        oh, of = h.reset(), f.reset()
        assert oh.dtype == torch.float16 and torch.equal(oh.view(torch.int16), of.half().view(torch.int16))
        g = torch.Generator(device="cuda").manual_seed(2)
        for _ in range(30):
            d = torch.randint(0, 6 * L * L + 1, (n,), device="cuda", generator=g, dtype=torch.int64)
            oh, rh, dh, ih = h.step(d)
            of, rf, df, i_f = f.step(d)
            assert oh.dtype == torch.float16 and torch.equal(oh.view(torch.int16), of.half().view(torch.int16))
            assert torch.equal(rh, rf) and torch.equal(dh, df)
            assert torch.equal(ih["action_mask"], i_f["action_mask"])
    finally:
        h.close()
        f.close()


@pytest.mark.parametrize("dtype", [np.float16, torch.float16])
def test_vector_env_f16_numpy(dtype):
    L, n, steps = 10, 8, 20
    seeds = SEED0 + np.arange(n)
    env = vector.VectorEnv("TD-def-small-v0", n, seed=SEED0, obs_dtype=dtype)
    bt = C.Batch(L, n, "def", 1, seeds, seeds, multi=bool(P.hyper_parameters.allow_multiple_actions))
    try:
        assert bt.initial_failed == [] and env.observation_space.dtype == np.float16
        ob = env.reset()
        assert isinstance(ob, np.ndarray) and ob.dtype == np.float16
        assert np.array_equal(ob.view(np.uint16), bt.obs().astype(np.float16).view(np.uint16))
        rng = np.random.RandomState(5)
        o32 = np.empty((n, 45, L, L), dtype=np.float32)
        for k in range(steps):
            d = rng.randint(0, 6 * L * L + 1, size=n).astype(np.int64)
            ob, rw, dn, _ = env.step(d)
            rw_c, dn_c = bt.step(d, None, obs=o32)
            assert ob.dtype == np.float16
            assert np.array_equal(ob.view(np.uint16), o32.astype(np.float16).view(np.uint16)), k
            assert np.array_equal(rw.view(np.uint64), rw_c.view(np.uint64)) and np.array_equal(dn, dn_c.astype(bool))
    finally:
        env.close()
        bt.close()
