"""The frame-skip reference recipe on the CPU oracle alone (oracle.td_cpu.Env, no GPU).

tests/test_gpu_frame_skip.py compares the device with this recipe bit for bit.  Its pass shows
that a board which finishes its episode at sub-step j of a macro step stops there and
auto-resets only if the recipe's episodes do end at every sub-step position j = 0 .. k-1:
asserted here, at least 5 ends per position in every case the GPU test runs -- but for the
even k of TD-atk / TD-2p, whose episodes end unevenly and which have floors of their own
(skiputil.check_ends)."""
import numpy as np
import pytest

import skiputil as S

FLOOR = 5


def recipe_ends(mode, k):
    """Episode ends per sub-step position of the recipe (skiputil.RECIPE) at frame skip k."""
    L, B = 10, S.RECIPE_BOARDS
    seeds, refs = S.make_refs(L, B, mode, S.recipe_cfg(), info=False)
    try:
        for b, ref in enumerate(refs):  # the phase shift: b % k single empty steps
            for _ in range(b % k):
                assert not ref.macro(1)["done"], "an episode ended during the phase shift"
        rng = np.random.RandomState(1)
        ends = np.zeros(k, dtype=int)
        for _ in range(S.recipe_steps(mode, k)):
            acts = S.draw_actions(rng, mode, B, L)
            for b, ref in enumerate(refs):
                d, a = S.act_of(acts, b)
                out = ref.macro(k, d, a)
                if out["done"]:
                    ends[out["ran"] - 1] += 1
        return seeds, ends
    finally:
        for ref in refs:
            ref.close()


@pytest.mark.parametrize("mode,k", S.RECIPE_CASES)
def test_recipe_ends_episodes_at_every_sub_step_position(mode, k):
    _, ends = recipe_ends(mode, k)
    print(mode, k, ends.tolist())
    S.check_ends(mode, k, ends)
    if mode == "def" or k == 3:  # k = 16, the maximum, included
        assert (ends >= FLOOR).all(), (mode, k, ends.tolist())


@pytest.mark.parametrize("autoreset", [False, True])
def test_config_run_reaches_what_it_is_there_for(autoreset):
    """td_set_config between macro steps (skiputil.ConfigTrace): without auto-reset at least 20
    enemies summoned in a sub-step >= 1 and towers built under at least 10 distinct configs --
    entities that must capture the launch's config epoch; with it at least 5 episodes ended."""
    tr = S.ConfigTrace(autoreset)
    print(autoreset, "late summons", tr.late_summons, "build configs", len(tr.build_cfgs), "ends", tr.ends)
    tr.check()


def test_macro_step_is_k_single_steps():
    """The reference itself: a macro step of 3 on one env equals three single steps on a twin
    (reward summed left to right, the last observation, the step counter), and stops at done."""
    cfg = S.recipe_cfg()
    (_, (x,)), (_, (y,)) = S.make_refs(10, 1, "def", cfg, info=False), S.make_refs(10, 1, "def", cfg, info=False)
    try:
        rng = np.random.RandomState(7)
        stopped = 0
        for _ in range(80):
            a = int(rng.randint(0, 601))
            m = x.macro(3, a)
            tot, last = None, None
            for j in range(3):
                last = y.macro(1, a if j == 0 else None)
                tot = last["reward"] if j == 0 else tot + last["reward"]
                if last["done"]:
                    break
            assert m["reward"].hex() == tot.hex() and m["done"] == last["done"] and m["ran"] == j + 1
            assert np.array_equal(m["obs"], last["obs"]) and m["ep_len"] == last["ep_len"]
            assert m["ep_ret"].hex() == last["ep_ret"].hex()
            stopped += int(m["done"] and m["ran"] < 3)
        assert stopped > 0
    finally:
        x.close()
        y.close()
