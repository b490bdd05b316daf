"""A retained step computes only what its written windows read (ObsWinTab::ntab, obs_need):
the channel-9 table is built only where a written window holds a unit of channel 9, and the
broadcast channels' f64 divisions run lane-parallel, one sequence per dependency level
(channel_scalars).  Nothing a caller sees may change.

A retained engine steps beside a retain_obs=False twin (same seeds, same actions) and every
output is compared as bytes after every one of 150 steps -- the recipe of
tests/test_gpu_obs_retain.py: its richer config, 40-step episodes, and its shapes:
L = 10 x 33 boards (eight consecutive boards cover all eight line misalignments -- the one
at which a window of the always-dirty class holds the last unit of channel 9 is among them
-- and 33 is odd), L = 20 TD-2p multi-action x 9, L = 30 x 9.  Boards of different road
lengths are neighbours in the grid (random seeds), and LDS is not cleared between
workgroups: a channel-9 table left over from another board would show in the bytes.

The run refuses itself unless the twin saw: an auto-reset, a tower built on a board with no
enemy, a board gaining its first enemy and a board losing its last, a base-LP loss and a
cost-bit flip (cost_def crossing a tower's price) -- and twice in mid-episode the observation
buffer is swapped (to a block full of 0xA5, then back to the first, which holds an observation
50 steps old): a launch that may not skip, between launches that do."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

import test_gpu_obs_retain as R  # noqa: E402  (its recipe: _engine, _cfg, _actions, _same, _snap)
from gym_TD import _lib  # noqa: E402

F32, F16 = torch.float32, torch.float16
SWAP_AT = (50, 100)  # 10 and 20 steps into an episode for a board that lived its 40 steps


class Events(R.Events):
    def __init__(self, L):
        super().__init__()
        self.price = np.array([c[0] for c in R._cfg(L).tower_cost], dtype=np.float64)
        self.calm_towers = self.cost_flips = self.swaps = 0

    def bits(self, cost_def):
        return (cost_def[:, None] >= self.price[None, :])

    def count(self, prev, cur, done):
        super().count(prev, cur, done)
        keep = ~done
        tw = (prev["n_tw"] < cur["n_tw"]) & (prev["n_en"] == 0) & (cur["n_en"] == 0)
        self.calm_towers += int((tw & keep).sum())
        self.cost_flips += int(((self.bits(prev["cost"]) != self.bits(cur["cost"])).any(axis=1) & keep).sum())

    def check(self):
        print("events: resets %d, towers %d (%d without enemies), first enemy %d, last enemy gone %d, LP losses %d, "
              "cost-bit flips %d, swaps %d" % (self.resets, self.towers, self.calm_towers, self.enemy_in, self.enemy_out,
                                               self.lp, self.cost_flips, self.swaps))
        assert self.resets > 0, "no board auto-reset"
        assert self.calm_towers > 0, "no tower was built on a board without enemies"
        assert self.enemy_in > 0 and self.enemy_out > 0, ("no board went from no enemy to some and back",
                                                          self.enemy_in, self.enemy_out)
        assert self.lp > 0, "no base lost life points"
        assert self.cost_flips > 0, "cost_def never crossed a tower's price"
        assert self.swaps == 2, "the buffer was not swapped and swapped back"


def _snap(eng):
    s = R._snap(eng)
    s["cost"] = eng.export_state()["hdr"]["cost_def"].copy()
    return s


def _swap(eng, buf):
    """The engine writes its observation to ``buf`` from now on; a retained engine is told that
    nothing is known of it (td_retain_obs), so its next launch may not skip."""
    torch.cuda.synchronize(eng.device)
    eng.obs = buf
    eng._io.obs = buf.data_ptr()
    if eng.retain_obs:
        _lib.check(_lib.lib.td_retain_obs(eng._h, buf.data_ptr()))
        assert _lib.lib.td_retained_obs(eng._h) == buf.data_ptr()


def _run(L, B, mode, multi, kernel, dtype, frame_skip=1, some_boards=False):
    a = R._engine(L, B, mode, multi, kernel, dtype, True)
    b = R._engine(L, B, mode, multi, kernel, dtype, False)
    try:
        assert a.retain_obs and not b.retain_obs and a.step_kernel == b.step_kernel == kernel
        if frame_skip > 1:
            a.set_frame_skip(frame_skip)
            b.set_frame_skip(frame_skip)
        a.reset_all()
        b.reset_all()
        R._same(a, b, "reset")
        first = {id(a): a.obs, id(b): b.obs}
        ev, prev, rng = Events(L), _snap(b), np.random.RandomState(11)
        for k in range(R.STEPS):
            if k in SWAP_AT:
                for e in (a, b):
                    if k == SWAP_AT[0]:
                        buf = torch.empty_like(e.obs)
                        R._bytes(buf).fill_(0xA5)
                    else:
                        buf = first[id(e)]  # as step SWAP_AT[0] - 1 left it
                    _swap(e, buf)
                ev.swaps += 1
            d, at = R._actions(rng, a)
            part = some_boards and k % 3 == 1
            if part:
                ids = np.flatnonzero(rng.random_sample(B) < 0.4).astype(np.int32)
                a.step_boards(ids, d, at)
                b.step_boards(ids, d, at)
            else:
                a.step(d, at)
                b.step(d, at)
            R._same(a, b, k)  # every board, every byte
            cur = _snap(b)
            if not part:  # (a partial step leaves the other boards' done flags as they were)
                ev.count(prev, cur, b.done.cpu().numpy().astype(bool))
            prev = cur
        ev.check()
        sa, sb = a.export_state(), b.export_state()
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), ("state", key)
        assert (a.flags() == 0).all() and (b.flags() == 0).all()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("kernel", ["small", "small2", "large"])
@pytest.mark.parametrize("L,B,mode,multi", R.SHAPES, ids=["L10-def", "L20-2p-multi", "L30-def"])
def test_needed_channels_only_equals_the_twin(L, B, mode, multi, kernel, dtype):
    _run(L, B, mode, multi, kernel, dtype)


def test_frame_skip_of_two():
    """td_skip_kernel shares the pieces: one observation after two board steps."""
    _run(10, 33, "def", False, "small", F32, frame_skip=2)


def test_through_step_boards():
    """Every third step names 40 % of the boards (td_step_boards): the others keep their rows."""
    _run(10, 33, "def", False, "small", F32, some_boards=True)
