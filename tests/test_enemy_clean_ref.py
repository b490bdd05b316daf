"""The premise of the enemy-touched rule (td_step_obs.h obs_dirty) on the CPU: on the Python
restatement a step without a summon, a sort that moved an enemy, a shot that landed or an
enemy entering a new cell never changes a byte of the 16 enemy planes -- in the recipe of
tests/test_gpu_enemy_clean.py and with the default config (bench.py's).  No GPU."""
import pytest

import enemyclean as E
from oracle import td_oracle as O


@pytest.mark.parametrize("recipe", ["test", "default"])
def test_quiet_steps_keep_the_enemy_planes(recipe):
    kw = {} if recipe == "test" else dict(cfg=O.Config(), hp=O.Hyper())
    tr = E.Trace(10, 48, "def", False, 200, **kw)
    c = tr.counts()
    assert c["missed"] == 0, c
    assert c["quiet"] >= 100 and c["quiet_slow"] >= 1, c  # margins change in every one of them
    assert min(c["summon"], c["shot"], c["move"]) >= 5, c
    # what the watcher calls quiet has its planes unchanged; the converse does not hold (an
    # enemy summoned and shot dead in one step)
    assert c["planes_same"] >= c["quiet"], c


def test_2p_multi_action_clusters():
    tr = E.Trace(20, 6, "2p", True, 60)
    c = tr.counts()
    assert c["missed"] == 0 and c["with_enemy"] > 0, c
