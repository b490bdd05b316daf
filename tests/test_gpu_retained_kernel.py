"""The step kernel is chosen per launch (td_kernel_choice.h retained_kernel_kind): a step into
the retained observation that leaves clean windows unwritten may run another kernel than a
step that writes every window.  Nothing a caller sees may depend on that.

Every test steps an engine whose two kinds differ beside a twin (same seeds, same actions) and
compares the observation bytes and every other output after every step.  The recipe, seeds and
shapes are those of tests/test_gpu_obs_retain.py: 40-step episodes on boards richer than the
defaults, so that within 150 steps every board auto-resets several times, tower lists change,
boards gain and lose enemies and bases lose life points -- counted on the twin and asserted.
Every REARM-th step the retained buffer is declared unknown again (td_retain_obs), so that a
launch of the full kind follows launches of the retained kind in mid-episode: the hand-over of
the board state and the opponent's hot record is exercised in both directions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

import test_gpu_obs_retain as R  # noqa: E402  (its recipe: _engine, _actions, _same, Events)
from gym_TD import _lib  # noqa: E402

REARM = 37
F32, F16 = torch.float32, torch.float16


def _stem(kind, dtype=F32):
    return {"large": "td_step_kernel", "small": "td_step_kernel_small", "small2": "td_step_kernel_small2"}[kind] + \
        ("_f16<" if dtype == F16 else "<")


def _split_engine(L, B, mode, multi, full, retained, dtype=F32, **kw):
    """A retained engine whose launches that write every window run ``full`` and whose skipping
    launches run ``retained``, through the hook."""
    e = R._engine(L, B, mode, multi, "auto", dtype, True, **kw)
    e.set_step_kernel(full)  # (forces both kinds)
    e.set_retained_step_kernel(retained)
    assert e.step_kernel == full and e.retained_step_kernel == retained
    assert e.step_kernel_name.startswith(_stem(full, dtype))
    return e


def _rearm(e):
    torch.cuda.synchronize(e.device)
    _lib.check(_lib.lib.td_retain_obs(e._h, e.obs.data_ptr()))


def _same_state(a, b):
    """Every exported array equal.  The opponent's stream is compared as CPython's getstate()
    (td_get_py_state, at most 64 boards spread over the batch): the raw record keeps how far a
    kernel has twisted the stream ahead of its position, and the large kernel twists lazily
    where the small kernels twist every step -- the same stream, another boundary word."""
    sa, sb = a.export_state(), b.export_state()
    for key in sa:
        if key != "opp_mt":
            assert np.array_equal(sa[key], sb[key]), ("state", key)
    for i in np.unique(np.linspace(0, a.B - 1, min(a.B, 64)).astype(int)):
        assert np.array_equal(a.get_py_state(i), b.get_py_state(i)), ("opponent stream", i)


def _run_pair(L, B, mode, multi, full, retained, dtype=F32, steps=R.STEPS, all_events=True):
    a = _split_engine(L, B, mode, multi, full, retained, dtype)
    b = R._engine(L, B, mode, multi, "auto", dtype, False)
    try:
        a.reset_all()
        b.reset_all()
        R._same(a, b, "reset")
        ev, prev, rng = R.Events(), R._snap(b), np.random.RandomState(11)
        seen = set()
        for k in range(steps):
            full_launch = k > 0 and k % REARM == 0
            if full_launch:
                _rearm(a)
            d, at = R._actions(rng, a)
            a.step(d, at)
            b.step(d, at)
            R._same(a, b, k)
            name = a.step_kernel_name
            if full_launch:
                assert name.startswith(_stem(full, dtype)), (k, name)
            elif k > 0:
                assert name.startswith(_stem(retained, dtype)), (k, name)
            seen.add(name)
            assert a.step_kernel == full and a.retained_step_kernel == retained
            cur = R._snap(b)
            ev.count(prev, cur, b.done.cpu().numpy().astype(bool))
            prev = cur
        assert len(seen) == (1 if full == retained else 2), seen
        if all_events:
            ev.check(B)
        else:
            assert ev.resets >= 2 * B, ev.resets
        _same_state(a, b)
        assert (a.flags() == 0).all() and (b.flags() == 0).all()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 1. kernel pairs, smallest shape
# (small2, small) and (large, small) are the pairs the rule's table produces; the others are kept
# as findings on the hand-over: any ordered pair is bit-exact.
@pytest.mark.parametrize("full,retained", [("small2", "small"), ("large", "small"), ("small", "small2"),
                                           ("small", "large"), ("small2", "large"), ("large", "small2")])
def test_kernel_pair_equals_the_twin(full, retained):
    _run_pair(10, 33, "def", False, full, retained)


# ------------------------------------------------------------------ 2. the name follows the launch
def test_name_alternates_and_the_kind_stays():
    a = _split_engine(10, 17, "def", False, "small2", "small")
    b = R._engine(10, 17, "def", False, "auto", F32, False)
    rng = np.random.RandomState(3)
    full, ret = "td_step_kernel_small2<10, 0, false>", "td_step_kernel_small<10, 0, false>"

    def step(want, where):
        d, at = R._actions(rng, a)
        a.step(d, at)
        b.step(d, at)
        R._same(a, b, where)
        assert a.step_kernel_name == want, (where, a.step_kernel_name)
        assert a.step_kernel == "small2" and a.retained_step_kernel == "small", where

    def reset_null(e):
        torch.cuda.synchronize(e.device)
        assert _lib.lib.td_reset(e._h, None, None, e._stream()) == 0

    try:
        assert a.step_kernel_name == full  # before the first step: a launch that writes every window
        a.reset_all()
        b.reset_all()
        _rearm(a)  # nothing known of the buffer: the first step writes every window
        step(full, "first")
        step(ret, "skipping 1")
        step(ret, "skipping 2")
        reset_null(a)
        reset_null(b)
        step(full, "after td_reset without obs")
        step(ret, "skipping 3")
        cfg = R._cfg()
        cfg.tower_cost = [[14, 14], [17, 17], [23, 23], [12, 12]]
        cfg.max_cost = 80
        a.set_config(cfg, R._hp(False))
        b.set_config(cfg, R._hp(False))
        step(full, "after td_set_config")
        step(ret, "skipping 4")
        # a kernel change names the full kernel again; AUTO gives both kinds back to their rules
        a.set_step_kernel("auto")
        assert a.step_kernel == "small2" and a.retained_step_kernel == "small2"  # 17 boards: within one round
        assert a.step_kernel_name == full
    finally:
        a.close()
        b.close()


def test_hook_refuses_what_td_set_step_kernel_refuses():
    e = R._engine(12, 5, "def", False, "auto", F32, True)
    try:
        assert e.step_kernel == "large" and e.retained_step_kernel == "large"
        for kind in ("small", "small2"):
            with pytest.raises(_lib.TDError, match="no small-batch step kernel"):
                e.set_retained_step_kernel(kind)
        assert _lib.lib.td_set_retained_step_kernel(e._h, 7) < 0
        e.set_retained_step_kernel("large")
        e.set_retained_step_kernel("auto")
        assert e.step_kernel == "large" and e.retained_step_kernel == "large"
    finally:
        e.close()


# ------------------------------------------------------------------ 3. the other builds
@pytest.mark.parametrize("L,mode,multi,dtype,full,all_events", [
    (10, "atk", False, F32, "small2", False),
    (10, "2p", False, F32, "small2", False),
    (10, "def", True, F32, "large", False),   # the pair the rule gives multi-action boards above a round
    (10, "2p", True, F32, "large", False),
    (20, "2p", True, F32, "small2", True),
    (30, "def", False, F32, "small2", True),
    (20, "2p", True, F16, "small2", True),
], ids=["L10-atk", "L10-2p", "L10-def-multi-large", "L10-2p-multi-large", "L20-2p-multi", "L30-def", "L20-2p-multi-f16"])
def test_other_builds(L, mode, multi, dtype, full, all_events):
    _run_pair(L, 9, mode, multi, full, "small", dtype, all_events=all_events)


# ------------------------------------------------------------------ 4. the real rule at its boundary
def test_rule_at_one_round_plus_one_wave():
    """8,256 boards: one round of the one-wave kernel on 256 CUs plus 64 boards.  A default engine
    (both kinds by their rules) against a twin forced to small2 for every launch."""
    L, B = 10, 8256
    a = R._engine(L, B, "def", False, "auto", F32, True)
    b = R._engine(L, B, "def", False, "small2", F32, True)
    try:
        assert b.step_kernel == "small2" and b.retained_step_kernel == "small2"
        on_256 = torch.cuda.get_device_properties(a.device).multi_processor_count == 256
        if on_256:
            assert a.step_kernel == "small2" and a.retained_step_kernel == "small"
        a.reset_all()
        b.reset_all()
        g = torch.Generator(device=a.device).manual_seed(5)
        for k in range(64):
            d = torch.randint(0, 6 * L * L + 1, (B,), device=a.device, generator=g, dtype=torch.int64)
            a.step(d)
            b.step(d)
            for name in R.OUTPUTS:
                ta, tb = getattr(a, name), getattr(b, name)
                assert (ta is None) == (tb is None), name
                assert ta is None or torch.equal(ta, tb), (name, k)
            if on_256 and k == 1:
                assert a.step_kernel_name == "td_step_kernel_small<10, 0, false>"
                assert b.step_kernel_name == "td_step_kernel_small2<10, 0, false>"
        assert (a.flags() == 0).all() and (b.flags() == 0).all()
        _same_state(a, b)
        assert int(a.export_state()["hdr"]["episodes"].sum()) >= B, "every board should have finished an episode"
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 5. unaffected paths
def test_frame_skip_keeps_the_skip_kernel():
    a = R._engine(10, 9, "def", False, "auto", F32, True)
    try:
        a.set_step_kernel("small2")
        a.set_retained_step_kernel("small")
        a.set_frame_skip(2)
        assert a.step_kernel_name == "td_skip_kernel<10, 0>"
        a.reset_all()
        rng = np.random.RandomState(2)
        for _ in range(4):
            a.step(*R._actions(rng, a))
            assert a.step_kernel_name == "td_skip_kernel<10, 0>"
        assert a.step_kernel == "small2" and a.retained_step_kernel == "small"
        a.set_frame_skip(1)
        assert a.step_kernel_name == "td_step_kernel_small2<10, 0, false>"
    finally:
        a.close()


def test_step_boards_between_split_steps():
    a = _split_engine(10, 33, "def", False, "small2", "small")
    b = R._engine(10, 33, "def", False, "small2", F32, True)
    try:
        sel = _lib.lib.td_step_boards_kernel_name(a._h).decode()
        a.reset_all()
        b.reset_all()
        rng = np.random.RandomState(9)
        for k in range(30):
            d, at = R._actions(rng, a)
            if k % 3 == 1:
                ids = np.flatnonzero(rng.random_sample(33) < 0.4).astype(np.int32)
                a.step_boards(ids, d, at)
                b.step_boards(ids, d, at)
            else:
                a.step(d, at)
                b.step(d, at)
            R._same(a, b, k)
        assert _lib.lib.td_step_boards_kernel_name(a._h).decode() == sel == "td_step_sel_kernel<10, 0, false>"
        assert a.step_kernel_name.startswith("td_step_kernel_small<")  # td_step's kernel, not the partial step's
    finally:
        a.close()
        b.close()


def test_kernel_timing_over_skipping_launches():
    a = _split_engine(10, 33, "def", False, "small2", "small")
    try:
        a.reset_all()
        rng = np.random.RandomState(4)
        a.step(*R._actions(rng, a))
        a.kernel_timing(3)
        for _ in range(3):
            a.step(*R._actions(rng, a))
            assert a.step_kernel_name == "td_step_kernel_small<10, 0, false>"
        t = a.kernel_times()
        assert len(t) == 3 and (t > 0).all()
    finally:
        a.close()
