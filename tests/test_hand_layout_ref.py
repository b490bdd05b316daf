"""Hand-made layouts on the host (no GPU): td_layout_from_roads against the oracle's map planes
on the catalogue of tests/handmaps.py, what the host refuses, the generated roads' place inside
the step kernels' 64-entry distance table, and -- on the oracle alone -- that each catalogue run
reaches what its map was drawn for, so the GPU comparison cannot pass vacuously."""
import functools

import numpy as np
import pytest

import handmaps as H
from oracle import canon
from oracle import td_oracle as O

from gym_TD import _lib
from gym_TD.engine import generate_layout, layout_planes

lib = _lib.lib
ROAD_ATTEMPTS = 1000  # td_kernels.h kRoadAttempts


@pytest.mark.parametrize("name", [n for n in H.MAPS if n != "deadend"])
def test_catalogue_records_match_oracle(name):
    """layout_planes(record) equals O.layout_from_roads on every catalogue map, and the record's
    max dist is the maximum of the finished distance plane (TDBoard.py:121-122) -- on `cross`,
    where road 1 overwrites road 0's farthest cell (17) with 9, that is 16."""
    L, roads = H.MAPS[name]
    H.check_roads(roads, L)
    rec = H.record(roads, L)
    m, start, end = O.layout_from_roads(roads, L)
    m2, s2, e2, nr2 = layout_planes(rec, L)
    assert np.array_equal(m, m2) and s2 == start and e2 == end and nr2 == len(roads)
    assert int(rec[3]) == int(m[4].max())
    assert int(rec[0]) == 0x7D1A0001 and int(rec[7]) == 0
    if name == "cross":
        assert int(rec[3]) == 16 and m[4, 6, 1] == 9 and m[5, 6, 1] == 0
    if name == "snake64":
        assert int(rec[3]) == 63 and len(roads[0]) == 64


@pytest.mark.parametrize("what,L,roads", [
    ("65 cells", 10, [H.path((9, 0), "U9 R1 D9 R1 U9 R1 D9 R6 U1 L5 U1 R5 U1 L5 U1")]),
    ("a cell twice, in a loop", 10, [H.path((2, 2), "R2 D2 L2 U2 R1")]),
    ("a cell twice in a row", 10, [[(2, 2), (2, 3), (2, 3), (2, 4)]]),
    ("an empty road", 10, [H.path((2, 2), "R3"), []]),
    ("a cell below the board", 10, [[(8, 4), (9, 4), (10, 4)]]),
    ("a negative cell", 10, [[(0, 1), (0, 0), (0, -1)]]),
])
def test_host_refuses_roads_outside_the_rule(what, L, roads):
    """td_layout_from_roads returns non-zero, with a message, and leaves rec[0] = 0 (no magic
    word: td_reset_layouts does not take it for a record) -- also in a buffer that held a
    valid record before."""
    if what == "a negative cell":  # (row * L + col = -1)
        assert roads[0][-1][0] * L + roads[0][-1][1] < 0
    rc, rec = H.try_record(roads, L)
    assert rc != 0 and int(rec[0]) == 0, what
    assert b"td_layout_from_roads" in lib.td_last_error()
    good = H.record(H.MAPS["border"][1], 10)
    assert int(good[0]) == 0x7D1A0001
    rc, _ = H.try_record(roads, L, good)
    assert rc != 0 and int(good[0]) == 0, what


@pytest.mark.parametrize("L", [8, 9, 31, 32])
def test_generated_roads_stay_inside_the_distance_table(L):
    """200 seeds per size, at both ends of what create_road_v2 can draw (8, 9) and of what the
    engine takes (31, 32): the native generator equals the oracle's create_road driven as
    Env.reset drives it -- status, layout digest, the stream's next draw -- and the record's
    max dist is at most 2L - 2 <= 62, inside the kernels' 64-entry table."""
    ok = 0
    for seed in range(200):
        w = np.zeros(625, np.uint32)
        lib.td_np_seed(_lib.ptr(w, _lib.ctypes.c_uint32), seed)
        st, rec = generate_layout(w, L, ROAD_ATTEMPTS)
        rs = np.random.RandomState(seed)
        nr = rs.randint(low=1, high=4)
        try:
            roads = O.create_road(rs, L, nr, ROAD_ATTEMPTS)
        except O.RoadGenError:
            roads = None
        assert (st == 0) == (roads is not None), (L, seed, st)
        assert lib.td_np_randint(_lib.ptr(w, _lib.ctypes.c_uint32), 0, 2 ** 31 - 1) == rs.randint(0, 2 ** 31 - 1), (L, seed)
        if roads is None:
            assert int(rec[0]) == 0, (L, seed)
            continue
        ok += 1
        m, start, end = O.layout_from_roads(roads, L)
        m2, s2, e2, nr2 = layout_planes(rec, L)
        assert nr2 == nr and canon.layout_digest(m2, s2, e2) == canon.layout_digest(m, start, end), (L, seed)
        assert int(rec[3]) == int(m[4].max()) <= 2 * L - 2, (L, seed, int(rec[3]))
        assert max(len(r) for r in roads) <= 2 * L - 1
    assert ok >= 100, (L, ok)


@pytest.mark.parametrize("L", [3, 33])
def test_create_refuses_sizes_outside_4_to_32(L):
    """td_create at L = 3 and L = 33: NULL and a message, before any device is touched."""
    c = _lib.TdConfig()
    lib.td_config_default(c)
    assert not lib.td_create(c, L, 4, 0, 0, 1, 0)
    assert b"map_size must be in [4, 32]" in lib.td_last_error()


# --------------------------------------------------------------------------
# the catalogue's conditions, on HandEnv alone
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _trace(case):
    return H.run_oracle(case)


def test_handenv_draws_nothing_and_keeps_the_opponent_stream():
    """HandEnv.reset(): no draw from np_random, the opponent's random.Random untouched, both
    cool-downs zero, num_roads the map's."""
    L, roads, envs = H.make_envs("merge3", 1)
    o = envs[0]
    np0, py0 = o.np_random.get_state(), o.rnd.getstate()
    o.attacker_cd = o.defender_cd = 3
    o.reset()
    assert (o.np_random.get_state()[1] == np0[1]).all() and o.np_random.get_state()[2] == np0[2]
    assert o.rnd.getstate() == py0
    assert (o.attacker_cd, o.defender_cd, o.num_roads, o._board.num_roads) == (0, 0, 3, 3)
    assert o._board.enemy_cap == 128 and o._board.tower_cap == 32 and o._board.refused is o.refused


@pytest.mark.parametrize("case", [c[0] for c in H.CASES])
def test_catalogue_runs_reach_their_conditions(case):
    """Each run, on the oracle alone: episodes end (by leaks and, over the catalogue, by the
    step limit), enemies leak, one stands on the farthest cell, one moves two or more cells
    through a turn in one step -- and what the map was drawn for."""
    tr = _trace(case)
    name = H.CASE[case][1]
    assert tr["refused"] == [0, 0], tr  # no list reaches its capacity: the device must end with flags 0
    assert tr["episodes"] >= 3, tr
    assert tr["leaks"] >= 5, tr
    assert tr["ends_by_leak"] >= 1, tr
    assert tr["on_maxdist"] >= 1, tr
    assert tr["turn_steps"] >= 1, tr
    if name in ("merge3", "snake64"):
        assert tr["dirs"] == {0, 1, 2, 3}, tr
    if name == "cross":
        assert tr["road0_on_road1_only"] >= 1, tr
    if name == "border" or name.startswith("tiny"):
        assert tr["clipped_towers"] >= 1 and tr["fail_pos"] >= 1, tr


def test_catalogue_ends_by_the_step_limit_too():
    assert sum(_trace(c[0])["ends_by_limit"] for c in H.CASES) >= 3


def test_bad_move_run_reaches_its_conditions():
    """The TD_FLAG_BAD_MOVE run on the oracle alone: every dead-end board notes a bad move, its
    episodes end (so the flag's clearing by a restart is compared), and no list fills up (the
    flag word holds nothing but bit 4)."""
    L, _, envs = H.bad_move_envs()
    noted = [0] * len(envs)
    rng = np.random.RandomState(L)
    for _ in range(H.BAD_MOVE_STEPS):
        _, aa = H.draw_actions(rng, "atk", envs, L)
        for b, o in enumerate(envs):
            done = o.step(None, aa[b])[2]
            if done:
                noted[b] += o._board.bad_move
                H.note_end(o)
                o.reset()
    assert all(noted[b] >= 2 for b in range(1, len(envs), 2)), noted  # episodes that ended with the flag set
    assert not any(noted[0::2]), noted
    assert all(o.refused == [0, 0] for o in envs)
    assert all(o.trace["episodes"] >= 3 for o in envs)


def test_stay_on_bad_move_is_opt_in():
    """On the dead-end map an enemy of road 1 reaches (5, 9), whose direction points off the
    board.  With the opt-in it stays there, its margin reduced by 1 each time it tries, and the
    board notes bad_move; without it the oracle keeps the reference's behaviour (here: the
    position leaves the map and numpy raises)."""
    L, roads = H.MAPS["deadend"]
    cfg, hp = H.config(), H.hyper()
    act = np.full((3, 8), 4, dtype=np.int64)
    act[1, 0] = 1  # one speed-1.0 enemy on road 1
    env = H.HandEnv(roads, L, O.MODE_ATK, 0, 5, cfg, hp, stay_on_bad_move=True)
    env.step(None, act)
    assert [e.loc for e in env._board.enemies if e.type == 1] == [[5, 9]] and not env._board.bad_move
    env.step(None, np.full((3, 8), 4, dtype=np.int64))
    e = [e for e in env._board.enemies if e.type == 1][0]
    assert e.loc == [5, 9] and e.margin == 0.0 and env._board.bad_move
    ref = H.HandEnv(roads, L, O.MODE_ATK, 0, 5, cfg, hp)
    ref.step(None, act)
    with pytest.raises(IndexError):
        ref.step(None, np.full((3, 8), 4, dtype=np.int64))
