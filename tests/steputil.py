"""The per-step comparison of one engine board with its oracle env, shared by
tests/test_gpu_envs.py (test_batched_modes_vs_oracle) and tests/test_gpu_hand_layouts.py.
Not a test module."""
import numpy as np

from oracle import canon


def _fc_list(row):
    return [int(v) for v in row if v >= 0]


def outputs(eng):
    """Every output of the engine's last step on the host, and the exported state."""
    host = lambda t: None if t is None else t.cpu().numpy()
    out = dict(obs=host(eng.obs), reward=host(eng.reward), done=host(eng.done), win=host(eng.win),
               allow_next=host(eng.allow_next), cooldowns=host(eng.cooldowns), real_def=host(eng.real_def),
               fail_def=host(eng.fail_def), real_atk=host(eng.real_atk), fail_atk=host(eng.fail_atk),
               state=eng.export_state())
    assert ((out["allow_next"] & 0xFC) == 0).all()  # AllowNextMove bits only (ABI 2: cool-downs have their own output)
    return out


def check_board(eng, out, b, o, stepped, mode, multi, tag, want_obs=None):
    """Board b of ``out`` (outputs(eng)) against oracle env ``o`` after ``stepped`` = o.step(...):
    reward bits, done, state digest, observation bytes, win, cool-downs, AllowNextMove and
    RealAction / FailCode.  ``want_obs``: the expected observation if it is not the oracle's
    own (e.g. its float16 rounding)."""
    L = eng.L
    wo, wr, wd, info = stepped
    ob, rw, dn, win, an, cdn = (out[k] for k in ("obs", "reward", "done", "win", "allow_next", "cooldowns"))
    rd, fd, ra, fa = (out[k] for k in ("real_def", "fail_def", "real_atk", "fail_atk"))
    assert canon.fhex(rw[b]) == canon.fhex(wr), tag
    assert bool(dn[b]) == wd, tag
    assert canon.state_digest(eng.board_state(b, out["state"])) == canon.state_digest(canon.oracle_state(o)), tag
    wo = wo if want_obs is None else want_obs
    assert np.array_equal(ob[b], wo), (tag, np.argwhere(ob[b] != wo)[:5].tolist())
    w = info["Win"]
    if isinstance(w, dict):
        w = w["Defender"] if mode != "atk" else w["Attacker"]
    assert (int(win[b]) if win[b] >= 0 else None) == (None if w is None else int(w)), tag
    assert (int(cdn[b]) & 15, int(cdn[b]) >> 4) == (min(o.attacker_cd, 15), min(o.defender_cd, 15)), tag
    anm = info["AllowNextMove"]
    if mode == "2p":
        assert bool(an[b] & 1) == anm["Attacker"] and bool(an[b] & 2) == anm["Defender"], tag
    elif mode == "atk":
        assert bool(an[b] & 1) == anm, tag
    else:
        assert bool(an[b] & 2) == anm, tag
    real, fc = info["RealAction"], info["FailCode"]
    if mode == "def":
        if multi:
            assert np.array_equal(rd[b], real), tag
        else:
            assert int(rd[b]) == int(real) and int(fd[b]) == int(fc), tag
    elif mode == "atk":
        assert np.array_equal(ra[b], real), tag
        assert _fc_list(fa[b]) == list(fc), tag
    else:
        if multi:
            assert np.array_equal(ra[b], real["Attacker"]) and np.array_equal(rd[b], real["Defender"]), tag
        else:
            if isinstance(real, dict):  # no defender success this step
                assert np.array_equal(ra[b], real["Attacker"]), tag
                assert int(rd[b]) == L * L * 6, tag
            else:  # TDMulti.py:257: the defender action replaced the dict
                assert int(rd[b]) == int(real), tag
            assert _fc_list(fa[b]) == fc["Attacker"] and int(fd[b]) == fc["Defender"], tag
