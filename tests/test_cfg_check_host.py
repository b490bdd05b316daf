"""The config check of td_create / td_set_config (gym-td_amd/csrc/td_cfg_check.h) without a GPU:
scripts/cfg_check_host.cpp walks every refusal and every accepted edge as a stand-alone host
program under the address and undefined-behaviour sanitizers, and every config
tests/cfgspace.py can draw converts to a td_config whose integer-typed fields are integers."""
import pytest

import cfgspace as S
from test_capi_tables_host import _run, cxx  # noqa: F401  (the compiler fixture and the runner)


def test_cfg_check_under_sanitizers(cxx, tmp_path):  # noqa: F811
    """Fractions, NaN and infinities in every double of the struct, the ends of every integer
    range, and the edge values the generator plants (all accepted)."""
    out = _run(cxx, tmp_path, "cfg_check")
    assert int(out.split("cfg_check: ")[1].split()[0]) >= 345


@pytest.mark.parametrize("regime", S.REGIMES)
def test_drawn_configs_are_representable(regime):
    """What draw() gives for the fields the device keeps as int32 is an int inside the range
    td_cfg_check.h accepts, for 100 draws per regime; gym_TD.params.to_c carries it over as is."""
    from gym_TD import params as P
    from oracle import td_oracle as O
    bounds = dict(frozen_time=(0, 255), tower_distance=(0, 15), base_LP=(1, 2 ** 31 - 1),
                  attacker_action_interval=(0, 2 ** 31 - 1), defender_action_interval=(0, 2 ** 31 - 1))
    for seed in range(100):
        ov = S.draw(seed, regime)
        c = P.to_c(O.Config(**ov), O.Hyper())
        for name, (lo, hi) in bounds.items():
            v = getattr(c, name)
            assert isinstance(ov[name], int) and v == ov[name] and lo <= v <= hi, (seed, name, v)
        assert c.max_tower_lv == ov["max_tower_lv"] and c.max_tower_lv in (0, 1)
        assert all(c.enemy_LP[t][l] > 0 for t in range(4) for l in range(2))
