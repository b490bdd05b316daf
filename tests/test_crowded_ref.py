"""The crowded-board scenarios on the CPU oracle alone (tests/crowdutil.py): they still
reach what tests/test_gpu_crowded.py compares the device on, and the oracle's optional
capacity rules (``enemy_cap`` / ``tower_cap``) change nothing until they refuse.

What the seeds in crowdutil.SCENARIOS gave when they were chosen, as the oracle counted it
(8 boards; t0-t3 = shots of tower type 0-3 at a target index >= 64):

  scenario       >64   =128  t0  t1  t2  t3  splash frozen kills lo-kill sort  head  h127
  sustained-2p   1649    0    1  60   0  25     0     25     0    693    168  17181    0
  sustained-atk  1514    0    0   0   1  15     1     15     2    304    164  10285    0
  full-atk       1122   81    0  13   0  53    38     53   123    357    188   1627   29
  full-def        992   82    0  20  18  17    73     17   150    367    256   1374    0
  full-2p-20     1385  113  164   8  13 107    29    107    74    141    246   3065   27
  full-atk-12    1249   76   78  21  15  34    40     34    80    336    366   1897   19
  overflow-atk   1300  429   86   6  21  95    92     95   202    388    388   6906   40
  overflow-2p    1043  217   43  18   0   2   135      2   203    546    114   3621   21

  full-2p-20: 645 board-steps on 32 towers, 1,776 builds refused, 43 destructs and 134
  upgrades on a full list, 44 builds after such a destruct.  towers-def: 1,085 / 681 / 114 /
  115 / 124.  overflow-atk: 5,517 summons refused on 7 of 8 boards; overflow-2p: 2,556 on 5.

A group head at index 127 (the last entry of a full list, the first of its type in its cell)
did not come up under the random attacker within these step counts; every fourth board of the
full-* TD-atk / TD-2p scenarios therefore has crowdutil._lone_last for an attacker, which
builds exactly that list in its first sixteen steps.
"""
import numpy as np
import pytest

import crowdutil as U
from gym_TD import masks
from oracle import canon
from oracle import td_oracle as O


def test_cap_fail_code_is_the_devices():
    assert O.FAIL_CAP == masks.FC_CAPACITY
    assert (U.ENEMY_CAP, U.TOWER_CAP) == (masks.ENEMY_CAP, masks.TOWER_CAP)


@pytest.fixture(scope="module")
def refs():
    """Every scenario once on the oracle (the expectations are dropped: only counters here)."""
    out = {}
    for scn in U.SCENARIOS:
        r = U.Reference(scn)
        r.steps = None
        out[scn.name] = r
    return out


@pytest.mark.parametrize("name", [s.name for s in U.SCENARIOS])
def test_scenario_reaches_its_branches(refs, name):
    """Each scenario's own floors, the list lengths the uncapped rules stay within, and no
    board of a crowd scenario finishing early (it would stop being compared)."""
    ref = refs[name]
    print(name, ref.counters, ref.refused)
    U.check_scenario(ref)
    assert ref.running >= ref.scn.B - 1


@pytest.mark.parametrize("name,k", U.SKIP_CASES)
def test_scenario_reaches_its_branches_at_frame_skip(name, k):
    """The same floors with the scenario run as steps // k macro steps at frame skip k (the
    policy once per macro step, crowdutil.Reference(scn, k)): what
    tests/test_gpu_frame_skip_crowded.py compares the td_skip_kernel family on.  Examples of
    what the oracle gave at k = 2: full-atk 20 board-steps on 128 enemies, 13 heads at index
    127 and 105 kills in the upper half; overflow-atk 2,345 refused summons on 7 of 8 boards;
    towers-def 772 board-steps on 32 towers, 216 refused builds, 47 destructs on a full list;
    overflow-2p refusals on exactly 4 of 8 boards."""
    ref = U.Reference(U.BY_NAME[name], k)
    ref.steps = None
    print(name, k, ref.counters, ref.refused)
    U.check_scenario(ref)
    assert ref.running >= ref.scn.B - 1


def test_uncapped_scenarios_cover_the_upper_half(refs):
    """Over the scenarios that need no cap on the oracle: every second-half branch of the
    step ran, many times over for the common ones."""
    tot = U.Counters()
    for scn in U.SCENARIOS:
        if not scn.capped:
            assert refs[scn.name].counters.max_enemies <= U.ENEMY_CAP
            assert refs[scn.name].counters.max_towers <= U.TOWER_CAP
            tot.add(refs[scn.name].counters)
    print(tot)
    assert tot.hi_steps >= 1000 and tot.full_steps >= 20
    assert all(n >= 1 for n in tot.hi_target), tot.hi_target
    for key in ("hi_splash", "hi_frozen", "hi_kills", "lo_kill_hi_live", "cross_sort", "hi_head", "head_127"):
        assert getattr(tot, key) >= 1, key


def _view(e):
    """One board-step as comparable values (reward bits, done, state, info, obs bytes)."""
    return (canon.fhex(e.reward), bool(e.done), e.digest, e.cds, repr(_plain(e.info)), canon.obs_digest(e.obs))


def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in sorted(x.items())}
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x if x is None or isinstance(x, bool) else (int(x) if isinstance(x, (int, np.integer)) else x)


def _side_by_side(scn, **caps_b):
    """Scenario `scn` on its own caps (a) and on `caps_b` (b), the same actions on both (drawn
    from a's boards): per step [(view a, view b, a's refusals so far)] per board, and b's envs."""
    _, ea = U.make_envs(scn)
    _, eb = U.make_envs(scn, **caps_b)
    rng = np.random.RandomState(scn.rng)
    out = []
    for k in range(scn.steps):
        da, aa = U.draw_actions(scn, rng, ea)
        wa, wb = U.step_envs(scn, ea, da, aa), U.step_envs(scn, eb, da, aa)
        out.append([(None if a is None else _view(a), None if b is None else _view(b), sum(o.refused))
                    for a, b, o in zip(wa, wb, ea)])
    return out, eb


@pytest.mark.parametrize("name", ["overflow-atk", "towers-def"])
def test_capped_equals_uncapped_until_the_first_refusal(name):
    """Same boards, same actions: the capped oracle is the uncapped one -- state digest,
    reward bits, done, info, observation -- up to each board's first refusal, and parts from
    it in that step.  (Not for ever: once the attacker has spent on both sides what the cap
    made it keep, two emptied boards can meet again.)"""
    scn = U.BY_NAME[name]
    hist, _ = _side_by_side(scn, enemy_cap=None, tower_cap=None)
    refused_boards = 0
    for b in range(scn.B):
        first = next((k for k, row in enumerate(hist) if row[b][2] > 0), None)
        for k, row in enumerate(hist):
            a, bb, _ = row[b]
            if a is None or bb is None:
                continue
            if first is None or k < first:
                assert a == bb, (name, b, k)
        if first is not None:
            refused_boards += 1
            a, bb, _ = hist[first][b]
            assert a[2] != bb[2], (name, b, first)  # the uncapped list holds the entry the cap refused
    assert refused_boards >= scn.B // 2


@pytest.mark.parametrize("name", ["full-atk"])
def test_caps_that_never_refuse_change_nothing(name):
    """A scenario the reference's rules keep within 128 enemies and 32 towers: the oracle
    with both caps set is identical throughout."""
    scn = U.BY_NAME[name]
    assert not scn.capped
    hist, capped = _side_by_side(scn, enemy_cap=U.ENEMY_CAP, tower_cap=U.TOWER_CAP)
    for k, row in enumerate(hist):
        for b, (a, bb, _) in enumerate(row):
            assert a == bb, (name, b, k)
    assert all(o.refused == [0, 0] for o in capped)
