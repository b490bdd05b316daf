"""Boards with 65-128 live enemies and full tower lists, against the oracle, bit for bit.

Lane l of a step wave owns enemies l and l + 64, and every phase of the step has a branch
of its own for the second one (td_step_rules.h board_step: the rank sort across the halves, the
target `m0 ? ctz(m0) : 64 + ctz(m1)`, the shots on lp[1], the compaction offset
popc(k0) + popc(k1 & lt); enemy_stats: group heads up to index 127 next to the 0xFF
sentinel; store_enemies and the three kernels' load paths beyond the 16 prefetched slots;
the tower parameter table that fills the enemy LP array's LDS to the byte at 32 towers).
The default config never brings a board there.  tests/crowdutil.py holds configs that do,
under the reference's own rules, and counts from the oracle's lists which of those branches
a bit-exact device must have taken; the same counters are asserted without a GPU in
tests/test_crowded_ref.py.

Every case compares, at every step and for every board still running: the reward bits and
done, the canonical digest of the exported state, every observation byte, RealAction,
FailCode, Win, AllowNextMove and the cool-downs; at the end the flag words -- 0 where the
oracle refused nothing, exactly TD_FLAG_EN_OVERFLOW / TD_FLAG_TW_OVERFLOW where its optional
caps (oracle/td_oracle.py enemy_cap / tower_cap, the device's documented refusal rules) did.
"""
import copy

import numpy as np
import pytest
import torch

import crowdutil as U
from oracle import canon

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import params as P  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402

ALL = ("large", "small", "small2")
# the scenario x kernel table (the generic-L build has the large kernel only; the 20x20
# two-wave kernel has a load path of its own)
CASES = [(s.name, k) for s in U.SCENARIOS
         for k in ({10: ALL, 20: ("large", "small2"), 12: ("large",)}[s.L])]


def _engine(scn, seeds, kernel):
    cfg = copy.deepcopy(P.config)
    for key, v in scn.cfg.items():
        setattr(cfg, key, copy.deepcopy(v))
    eng = TDEngine(scn.L, scn.B, scn.mode, scn.multi, scn.difficulty, np_seeds=seeds, py_seeds=seeds,
                   autoreset=False, cfg=cfg, step_kernel=kernel)
    assert eng.step_kernel == kernel
    return eng


def _fc_list(row):
    return [int(v) for v in row if v >= 0]


class _Out(object):
    """One step's outputs on the host."""

    def __init__(self, eng):
        cp = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        self.obs, self.reward, self.done = cp(eng.obs), cp(eng.reward), cp(eng.done)
        self.win, self.allow, self.cds = cp(eng.win), cp(eng.allow_next), cp(eng.cooldowns)
        self.real_def, self.fail_def = cp(eng.real_def), cp(eng.fail_def)
        self.real_atk, self.fail_atk = cp(eng.real_atk), cp(eng.fail_atk)
        self.state = eng.export_state()


def _check_board(scn, eng, out, b, w, tag):
    """Board b of `out` against the oracle's Expect `w` (as test_batched_modes_vs_oracle)."""
    L, mode, multi = scn.L, scn.mode, scn.multi
    assert canon.fhex(out.reward[b]) == canon.fhex(w.reward), tag
    assert bool(out.done[b]) == w.done, tag
    assert canon.state_digest(eng.board_state(b, out.state)) == w.digest, tag
    assert np.array_equal(out.obs[b], w.obs), (tag, np.argwhere(out.obs[b] != w.obs)[:5].tolist())
    win = w.info["Win"]
    if isinstance(win, dict):
        win = win["Defender"] if mode != "atk" else win["Attacker"]
    assert (int(out.win[b]) if out.win[b] >= 0 else None) == (None if win is None else int(win)), tag
    assert (int(out.cds[b]) & 15, int(out.cds[b]) >> 4) == (min(w.cds[0], 15), min(w.cds[1], 15)), tag
    an, anm = out.allow[b], w.info["AllowNextMove"]
    assert (an & 0xFC) == 0, tag
    if mode == "2p":
        assert bool(an & 1) == anm["Attacker"] and bool(an & 2) == anm["Defender"], tag
    elif mode == "atk":
        assert bool(an & 1) == anm, tag
    else:
        assert bool(an & 2) == anm, tag
    real, fc = w.info["RealAction"], w.info["FailCode"]
    if mode == "def":
        if multi:
            assert np.array_equal(out.real_def[b], real), tag
        else:
            assert int(out.real_def[b]) == int(real) and int(out.fail_def[b]) == int(fc), tag
    elif mode == "atk":
        assert np.array_equal(out.real_atk[b], real), tag
        assert _fc_list(out.fail_atk[b]) == list(fc), tag
    elif multi:
        assert np.array_equal(out.real_atk[b], real["Attacker"]), tag
        assert np.array_equal(out.real_def[b], real["Defender"]), tag
    else:
        if isinstance(real, dict):  # no defender success this step
            assert np.array_equal(out.real_atk[b], real["Attacker"]), tag
            assert int(out.real_def[b]) == L * L * 6, tag
        else:  # TDMulti.py:257: the defender action replaced the dict
            assert int(out.real_def[b]) == int(real), tag
        assert _fc_list(out.fail_atk[b]) == fc["Attacker"] and int(out.fail_def[b]) == fc["Defender"], tag


def _step(eng, da, aa):
    eng.step(def_act=None if da is None else torch.from_numpy(da),
             atk_act=None if aa is None else torch.from_numpy(aa))


@pytest.mark.parametrize("name,kernel", CASES)
def test_crowded_boards_vs_oracle(name, kernel):
    """One scenario on one step kernel.  The scenario's floors on the oracle's counters are
    asserted first, from the very envs the device is compared with: a pass means the
    second-half branches the scenario is there for have run, and run right."""
    scn = U.BY_NAME[name]
    ref = U.reference(scn)
    print(name, kernel, ref.counters)
    U.check_scenario(ref)
    eng = _engine(scn, ref.seeds, kernel)
    try:
        _, failed = eng.reset()
        assert not failed
        compared = 0
        for k, (da, aa, want) in enumerate(ref.steps):
            _step(eng, da, aa)
            out = _Out(eng)
            for b, w in enumerate(want):
                if w is not None:  # (else: finished in an earlier step, no auto-reset here)
                    _check_board(scn, eng, out, b, w, (name, kernel, k, b))
                    compared += 1
        assert compared >= (scn.B - 1) * scn.steps
        assert eng.flags().tolist() == ref.flags(), (eng.flags().tolist(), ref.refused)
        if not scn.capped:
            assert (eng.flags() == 0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("kernel", ALL)
def test_export_import_roundtrip_above_64_enemies(kernel):
    """td_export_state / td_import_state with the upper half of the enemy list in use: the
    sustained TD-2p crowd is stepped until all boards but two hold more than 64 enemies, exported
    and imported into a fresh engine (other seeds, never stepped); both then take the
    scenario's next 20 steps and every output tensor and the exported state stay identical
    (the first engine is the one test_crowded_boards_vs_oracle pins to the oracle)."""
    scn = U.BY_NAME["sustained-2p"]
    ref = U.reference(scn)
    crowded = lambda n: sum(v > U.HALF for v in n)  # noqa: E731
    k0 = next(k for k, n in enumerate(ref.n_enemies) if crowded(n) >= scn.B - 2)
    assert k0 + 21 <= scn.steps and all(crowded(n) >= scn.B // 2 for n in ref.n_enemies[k0:k0 + 21])
    a = _engine(scn, ref.seeds, kernel)
    b = _engine(scn, [s + 1000 for s in ref.seeds], kernel)
    try:
        a.reset()
        b.reset_all()
        for k in range(k0 + 1):
            _step(a, ref.steps[k][0], ref.steps[k][1])
        st = a.export_state()
        assert int((st["hdr"]["n_en"] > U.HALF).sum()) >= scn.B - 2
        b.import_state(st)
        for i in range(scn.B):
            assert canon.state_digest(b.board_state(i)) == canon.state_digest(a.board_state(i, st)), i
        names = ("obs", "reward", "done", "win", "allow_next", "cooldowns", "real_def", "fail_def", "real_atk", "fail_atk")
        for k in range(k0 + 1, k0 + 21):
            _step(a, ref.steps[k][0], ref.steps[k][1])
            _step(b, ref.steps[k][0], ref.steps[k][1])
            for nm in names:
                assert torch.equal(getattr(a, nm), getattr(b, nm)), (kernel, k, nm)
            sa, sb = a.export_state(), b.export_state()
            for i in range(scn.B):
                assert canon.state_digest(a.board_state(i, sa)) == canon.state_digest(b.board_state(i, sb)), (k, i)
            assert int(sa["hdr"]["n_en"].max()) > U.HALF
        assert (a.flags() == 0).all() and (b.flags() == 0).all()
    finally:
        a.close()
        b.close()
