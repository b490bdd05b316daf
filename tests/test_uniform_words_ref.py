"""The cases of tests/uniformwords.py on the CPU oracle alone: each still reaches the events it
is there for (the floors of its `needs`), so that the device comparison on it
(tests/test_gpu_uniform_words.py) compares what it claims to.  No GPU."""
import numpy as np
import pytest

import uniformwords as W


@pytest.mark.parametrize("case", W.CASES, ids=repr)
def test_case_reaches_its_events(case):
    _, envs, cfg, hp = W.make_envs(case)
    led = W.Ledger()
    rng = np.random.RandomState(case.rng)
    with W.counting(led):
        for k in range(case.steps):
            W.apply_switch(case, k, cfg, hp)
            run = W.live(case, envs)
            da, aa = W.draw_actions(case, rng, envs)
            for b in run:
                envs[b].step(*W.act_of(case, da, aa, b))
    W.check_needs(case, led)
    assert len(W.live(case, envs)) >= W.B // 2, "most boards are compared to the end"
