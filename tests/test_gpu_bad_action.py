"""Out-of-range actions on the device (TD_FLAG_BAD_ACTION), against the oracles, bit for bit.

Every step kernel has its own text for the rule of include/tdstep.h (td_board_flag): the
discrete defender's int64 put together from two prefetched 32-bit words (td_step_body.h,
td_step_skip.h), the attacker's 24 entries (td_step_rules.h attacker_actions), the
multi-action planes' 16-byte and scalar paths (scan_fold) and, in the two-wave kernels, the
second wave's verdict handed over through LDS.  tests/badact.py sends -1, -2^63, 2^31, one
past the space and 2^32 + a with an ``a`` that would change the board right now, to even
boards on a fixed schedule, cooling down or not, and steps the oracles with the sanitised
action; tests/test_bad_action_ref.py shows on the CPU that each run holds at least 8 such
live ``a``.  A bad action on an ordinary step is also the way into store_board's
``u.flags != S.flags0`` term.

Compared at every step and for every board: reward bits, done, win, allow_next, cooldowns,
the episode's return and length, real_* and fail_*, every observation byte, the state digest
and the flag word: 4 from the first step that carried a bad value for the board, not one step
earlier, across auto-resets, 0 on the boards that never got one.  At the end explicit resets:
they clear the flags of the boards they reset (td_reset.hip reset_one, keep_flags) and of
no other.
"""
import numpy as np
import pytest
import torch

import badact as A
from oracle import canon

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD.engine import TDEngine  # noqa: E402

F32, F16 = torch.float32, torch.float16
KERNELS = {10: ("large", "small", "small2"), 20: ("large", "small2"), 12: ("large",), 11: ("large",)}
# discrete: every kernel of the side in float32, float16 too at L = 10
DISCRETE = [(m, L, kern, dt) for (m, _, L) in A.DISCRETE for dt in ((F32, F16) if L == 10 else (F32,))
            for kern in KERNELS[L]]
# multi-action: L = 20 for the second-wave fold and its hand-over, L = 11 for scan_fold's
# scalar path (odd L^2); off: def_act and real_def 8 bytes into their allocations (the scalar
# paths of scan_fold and scan_write_real at even L^2)
MULTI = [(m, L, kern, off) for (m, _, L) in A.MULTI for off in ((0, 8) if L == 10 else (0,)) for kern in KERNELS[L]]
GUARD = 0x5A5A5A5A5A5A5A5A


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _offset(t, guard):
    """A copy of int64 tensor ``t`` 8 bytes into an allocation of its own, a guard word on
    either side: (the allocation, the view)."""
    buf = torch.full((t.numel() + 2,), guard, dtype=torch.int64, device="cuda")
    view = buf[1:-1].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + 8 and view.is_contiguous()
    return buf, view


def _compare(eng, tr, s, f16):
    multi, mode = tr.multi, tr.mode
    ob = eng.obs.cpu().numpy()
    host = {n: getattr(eng, n).cpu().numpy() for n in ("reward", "done", "win", "allow_next", "cooldowns", "ep_return", "ep_len")}
    for n in ("real_def", "fail_def", "real_atk", "fail_atk"):
        t = getattr(eng, n)
        host[n] = None if t is None else t.cpu().numpy()
    st = eng.export_state()
    flags = eng.flags()
    assert np.array_equal(st["hdr"]["flags"], flags), s
    for b, o in enumerate(tr.outs[s]):
        w = (mode, multi, tr.L, s, b)
        assert int(flags[b]) == int(tr.flags[s][b]), (w, "flags", flags.tolist(), tr.flags[s].tolist())
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
        assert canon.state_digest(eng.board_state(b, st)) == o["digest"], (w, "state")
        if mode != "atk":
            assert np.array_equal(host["real_def"][b], o["real_def"]), (w, "real_def")
            if not multi:
                assert int(host["fail_def"][b]) == o["fail_def"], (w, "fail_def")
        if mode != "def":
            assert np.array_equal(host["real_atk"][b], o["real_atk"]), (w, "real_atk")
            if not multi:
                assert np.array_equal(host["fail_atk"][b], o["fail_atk"]), (w, "fail_atk")


def _run(tr, kernel="large", dtype=F32, off=0):
    A.check_trace(tr)  # (tests/test_bad_action_ref.py, without a GPU)
    B, L, mode, multi = A.B, tr.L, tr.mode, tr.multi
    f16 = dtype == F16
    eng = TDEngine(L, B, mode, multi, 1, np_seeds=tr.seeds, py_seeds=tr.seeds, autoreset=True, cfg=tr.cfg,
                   step_kernel=kernel, obs_dtype=dtype, frame_skip=tr.k)
    try:
        assert eng.step_kernel == kernel
        _, failed = eng.reset()
        assert not failed
        ob = eng.obs.cpu().numpy()
        for b, w in enumerate(tr.first):
            assert np.array_equal(_bits(ob[b]), _bits(w.astype(np.float16) if f16 else w)), ("first obs", b)
        real_buf = None
        if off:
            real_buf, eng.real_def = _offset(eng.real_def, GUARD)
            eng._io.real_def = eng.real_def.data_ptr()
        for s, (d, a) in enumerate(tr.acts):
            d = None if d is None else torch.from_numpy(d).cuda()
            if off:
                act_buf, d = _offset(d, 0)
            eng.step(def_act=d, atk_act=None if a is None else torch.from_numpy(a))
            _compare(eng, tr, s, f16)
            if off:
                assert int(real_buf[0]) == GUARD and int(real_buf[-1]) == GUARD, s
        # explicit resets clear the flags of the boards they reset, and of no other
        before = eng.flags()
        mask = np.zeros(B, dtype=np.uint8)
        mask[0:B:4] = 1  # half of the flagged boards
        _, failed = eng.reset(mask)
        want = np.where((mask == 1) & ~np.isin(np.arange(B), failed), 0, before)
        assert (before[mask == 1] == A.FLAG_BAD_ACTION).all() and len(failed) < mask.sum()
        assert np.array_equal(eng.flags(), want), (eng.flags().tolist(), want.tolist(), failed)
        eng.reset_all()
        assert (eng.flags() == 0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("mode,L,kernel,dtype", DISCRETE)
def test_discrete_actions_out_of_range(mode, L, kernel, dtype):
    _run(A.trace(mode, False, L), kernel, dtype)


@pytest.mark.parametrize("mode,L,kernel,off", MULTI)
def test_multi_action_flags_out_of_range(mode, L, kernel, off):
    _run(A.trace(mode, True, L), kernel, off=off)


@pytest.mark.parametrize("mode,L", [(m, L) for (m, _, L) in A.SKIP])
def test_out_of_range_at_frame_skip(mode, L):
    """k = 3: sub-step 0 takes the caller's action, TD_FLAG_BAD_ACTION included; the flag is there
    after the macro step, also where that macro step ends the episode at sub-step 0, 1 or 2."""
    tr = A.trace(mode, False, L, A.SKIP_K)
    assert all(n >= 1 for n in tr.ends_bad), tr.ends_bad
    _run(tr)
