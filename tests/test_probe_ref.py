"""The rule of td_probe on the CPU (no GPU): gym_TD.sampling.reference_probe on the Python oracle.
reps = 1 is reference_playout; replica r is reference_playout at ticket + r * steps on a copy; the
source env -- its state and both of its streams -- is the same before and after."""
import copy

import numpy as np
import pytest

import maskutil as M
import playoutref as PR
from gym_TD import sampling as S

SEED = 9


def _whole(env):
    """Everything of an oracle env a probe could have disturbed: the canonical state and both
    streams."""
    np_state = env.np_random.get_state()
    return (str(M.oracle_state(env)), env.rnd.getstate(), np_state[1].tobytes(), np_state[2])


def _same_result(a, b):
    assert np.float64(a["reward"]).view(np.uint64) == np.float64(b["reward"]).view(np.uint64)
    assert (a["done"], a["steps_run"], a["events"]) == (b["done"], b["steps_run"], b["events"])
    assert np.array_equal(a["first_def"], b["first_def"]) and np.array_equal(a["first_atk"], b["first_atk"])


def _envs(mode, n=3, limit=23):
    cfg, hp = PR.anchor_config()
    hp.max_episode_steps = limit
    seeds, envs = M.ok_seeds(10, n, 500, PR.MODES[mode], cfg=cfg, hp=hp)
    for b, env in enumerate(envs):  # into the episode, each board elsewhere
        if S.reference_playout(env, M.oracle_state, 10, cfg, hp, mode, SEED, 1 << 20, b, 4 + 5 * b, 0.3, 0.3)["done"]:
            M.reset_ok(env)
    return cfg, hp, envs


@pytest.mark.parametrize("mode", ["def", "atk", "2p"])
def test_one_replica_is_the_playout(mode):
    cfg, hp, envs = _envs(mode)
    for b, env in enumerate(envs):
        before = _whole(env)
        (got,) = S.reference_probe(env, 7, 1, M.oracle_state, 10, cfg, hp, mode, SEED, 40, b, 0.3, 0.3)
        assert _whole(env) == before
        want = S.reference_playout(env, M.oracle_state, 10, cfg, hp, mode, SEED, 40, b, 7, 0.3, 0.3)
        _same_result(got, want)


@pytest.mark.parametrize("mode", ["def", "atk", "2p"])
def test_replica_r_is_the_playout_at_its_ticket_on_a_copy(mode):
    """Across the 2^64 wrap of the ticket; replicas end episodes and do not; they differ."""
    cfg, hp, envs = _envs(mode)
    steps, reps, ticket = 9, 5, S.M64 - 20
    done, differ = set(), 0
    for b, env in enumerate(envs):
        before = _whole(env)
        got = S.reference_probe(env, steps, reps, M.oracle_state, 10, cfg, hp, mode, SEED, ticket, b, 0.3, 0.3)
        assert len(got) == reps and _whole(env) == before
        for r in range(reps):
            twin = copy.deepcopy(env)
            want = S.reference_playout(twin, M.oracle_state, 10, cfg, hp, mode, SEED, (ticket + r * steps) & S.M64, b,
                                       steps, 0.3, 0.3)
            _same_result(got[r], want)
            done.add(bool(want["done"]))
        differ += len({(g["reward"], str(g["events"])) for g in got}) > 1
        assert _whole(env) == before
    assert done == {False, True} and differ > 0, (done, differ)


def test_source_env_compares_equal_and_can_go_on():
    """The probed env steps on exactly as a copy taken before the probe."""
    cfg, hp, envs = _envs("def", n=1, limit=60)
    env = envs[0]
    twin = copy.deepcopy(env)
    S.reference_probe(env, 12, 4, M.oracle_state, 10, cfg, hp, "def", SEED, 0, 0)
    assert _whole(env) == _whole(twin)
    a = S.reference_playout(env, M.oracle_state, 10, cfg, hp, "def", SEED, 100, 0, 10)
    b = S.reference_playout(twin, M.oracle_state, 10, cfg, hp, "def", SEED, 100, 0, 10)
    _same_result(a, b)
    assert _whole(env) == _whole(twin)
