"""The rule of td_sample_actions on the CPU (no GPU): gym_TD.sampling against known answers, the
same rule as C++ (csrc/td_sample.h, with td_call_check.h's io check) run as a stand-alone program
under the address and undefined-behaviour sanitizers, reference_sample on hand-made masks, the
uniformity of the draws, and brute force on the CPU oracle: along runs driven by
reference_sample over reference_masks alone, every sampled action is what the env executes."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import maskutil as M
import sampleutil as U
from gym_TD import sampling as S
from gym_TD.masks import reference_masks
from oracle import td_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
L = 10
NC = L * L
A = 6 * NC
MAXU = 2 ** 32 - 1


# ------------------------------------------------------------------------------ known answers
def test_known_answers():
    assert S.sm(0) == U.SM0
    for args, w, u in U.KNOWN:
        assert S.word(*args) == w, args
        assert S.u32(*args) == u == w >> 32, args


def test_rule_as_a_host_program_under_sanitizers(tmp_path):
    """scripts/sample_rule_host.cpp: the known answers, the idle and pick arithmetic at both ends
    of u, and the io check's verdicts with their whole messages, in refusal order; then the
    program's word for a handful of draws against the Python mirror."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + FLAGS + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "sample_rule_host")
    cc = subprocess.run([cxx] + FLAGS + ["-o", exe, os.path.join(ROOT, "scripts", "sample_rule_host.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.search(r"^sample_rule: \d+ cases ok$", run.stdout, re.M), run.stdout
    rng = np.random.RandomState(5)
    for _ in range(8):
        seed, ticket = ((int(hi) << 32) | int(lo) for hi, lo in rng.randint(0, 2 ** 32, size=(2, 2), dtype=np.int64))
        b, j = int(rng.randint(0, 2 ** 31)), int(rng.randint(0, 4))
        out = subprocess.run([exe, str(seed), str(ticket), str(b), str(j)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        w, u = out.stdout.split()
        assert int(w, 16) == S.word(seed, ticket, b, j) and int(u) == S.u32(seed, ticket, b, j)


# ------------------------------------------------------------------------ hand-made masks
def _def_mask(legal, multi=False):
    m = np.zeros(A, dtype=np.uint8)
    m[list(legal)] = 1
    return m.reshape(6, L, L) if multi else np.concatenate([m, np.ones(1, dtype=np.uint8)])


def _sample(dm, am, b=0, ticket=0, def_idle=0, atk_idle=0, multi=False, seed=9):
    return S.reference_sample(dm, am, seed, ticket, b, def_idle, atk_idle, L, multi)


def test_empty_mask_is_the_noop():
    for b in range(50):
        d, a, dn, an = _sample(_def_mask([]), None, b=b)
        assert d == A and dn == 0 and a is None and an is None


def test_one_legal_entry_at_either_end():
    for k in (0, A - 1):
        for b in range(50):
            d, _, dn, _ = _sample(_def_mask([k]), None, b=b)
            assert d == k and dn == 1, (k, b)  # def_idle = 0: the only candidate, always


def test_all_legal_follows_the_pick_word():
    for b in range(200):
        d, _, dn, _ = _sample(_def_mask(range(A)), None, b=b, ticket=3)
        assert dn == A and d == (S.u32(9, 3, b, S.DEF_PICK) * A) >> 32 and 0 <= d < A
    # the no-op of the discrete row is no candidate
    assert _sample(np.ones(A + 1, dtype=np.uint8), None)[2] == A


def test_closed_cooldown_gives_no_candidate():
    """reference_masks of a state with the cool-down closed: only the no-op is legal."""
    cfg, hp = M.config(M.RICH), M.hyper()
    st = {"steps": 5, "cost_def": 500.0, "cost_atk": 500.0, "attacker_cd": 3, "defender_cd": 2, "num_roads": 2,
          "towers": [(0, 0, 1, 1, 0.0)], "enemies": [], "map6": [0] * NC}
    dm, _, am = reference_masks(st, L, cfg, hp, "2p", False)
    d, a, dn, an = _sample(dm, am)
    assert d == A and dn == 0 and an == 0 and (a == 4).all()
    st["defender_cd"], st["attacker_cd"] = 1, 1
    dm, _, am = reference_masks(st, L, cfg, hp, "2p", False)
    d, a, dn, an = _sample(dm, am)
    assert dn > 0 and d < A and dm[d] == 1 and an == 8 and U.atk_pick(a) is not None


def test_multi_action_sets_one_flag():
    legal = [3, 150, 599]
    seen = set()
    for b in range(100):
        d, _, dn, _ = _sample(_def_mask(legal, True), None, b=b, multi=True)
        assert d.shape == (6, L, L) and d.dtype == np.int64 and d.sum() == 1 and dn == 3
        seen.add(int(np.flatnonzero(d.reshape(-1))[0]))
    assert seen == set(legal)
    d, _, dn, _ = _sample(_def_mask([], True), None, multi=True)
    assert not d.any() and dn == 0
    d, _, dn, _ = _sample(_def_mask(legal, True), None, multi=True, def_idle=MAXU)
    assert dn == 3 and (not d.any()) == (S.u32(9, 0, 0, S.DEF_IDLE) < MAXU)


@pytest.mark.parametrize("roads", [1, 2, 3])
def test_attacker_roads(roads):
    am = np.zeros((3, 5), dtype=np.uint8)
    am[:, 4] = 1
    am[:roads, :4] = 1
    am[0, 2] = 0  # one type too dear
    seen = set()
    for b in range(300):
        _, a, _, an = _sample(None, am, b=b)
        assert a.shape == (3, 8) and a.dtype == np.int64 and an == 4 * roads - 1
        rt = U.atk_pick(a)
        assert rt is not None and am[rt[0], rt[1]] == 1
        k = sorted(r * 4 + t for r in range(roads) for t in range(4) if am[r, t])
        assert rt[0] * 4 + rt[1] == k[(S.u32(9, 0, b, S.ATK_PICK) * an) >> 32]
        seen.add(rt)
    assert len(seen) == 4 * roads - 1


def test_idle_probability_ends():
    dm = _def_mask(range(0, A, 7))
    idled = 0
    for b in range(300):
        assert _sample(dm, None, b=b, def_idle=0)[0] != A  # 0: only when nothing is legal
        d = _sample(dm, None, b=b, def_idle=MAXU)[0]
        assert (d == A) == (S.u32(9, 0, b, S.DEF_IDLE) < MAXU)  # not "all": u = 2^32 - 1 still acts
        idled += d == A
    assert idled >= 299
    assert S.idle_units(0.0) == 0 and S.idle_units(1.0) == MAXU and S.idle_units(0.3) == U.IDLE_03
    assert S.idle_units(MAXU) == MAXU and S.idle_units(0) == 0
    for bad in (-0.1, 1.5, -1, 2 ** 32):
        with pytest.raises(ValueError):
            S.idle_units(bad)


# ----------------------------------------------------------------------------- uniformity
@pytest.mark.parametrize("n,tickets,cap", [(7, 70000, 22.46), (301, 60200, 381.4)])
def test_picks_are_uniform(n, tickets, cap):
    """chi^2 of the pick among n candidates over tickets 0 .. tickets - 1 at (seed 12345, board 0)
    below the 99.9 % quantile of n - 1 degrees of freedom (deterministic: 5.6 and 307.5)."""
    counts = np.zeros(n, dtype=np.int64)
    for t in range(tickets):
        counts[(S.u32(12345, t, 0, S.DEF_PICK) * n) >> 32] += 1
    x = U.chi2(counts)
    print("chi2 n=%d: %.2f" % (n, x))
    assert x < cap, x


def test_idle_rate():
    """def_idle = 0x4CCCCCCC over boards 0 .. 65,535 at ticket 0 (seed 12345): 0.3 +- 0.008 (4.5 sigma)."""
    rate = sum(S.u32(12345, 0, b, S.DEF_IDLE) < U.IDLE_03 for b in range(65536)) / 65536.0
    print("idle rate: %.4f" % rate)
    assert abs(rate - 0.3) <= 0.008, rate


# ------------------------------------------------------------------ brute force on the oracle
def _summoned(fc_atk, real_atk, rt):
    return len(fc_atk) > rt[0] and fc_atk[rt[0]] == 0 and int(real_atk[rt[0]][0]) == rt[1]


@pytest.mark.parametrize("mode,multi", [("def", False), ("def", True), ("atk", False), ("2p", False)])
def test_sampled_action_is_what_the_oracle_executes(mode, multi):
    """100 steps of one 10x10 env driven by reference_sample over reference_masks (idle 0.3 on
    both sides): RealAction is the sampled action and FailCode 0, from the env's info."""
    omode = {"def": O.MODE_DEF, "atk": O.MODE_ATK, "2p": O.MODE_2P}[mode]
    cfg = M.config(M.RICH) if mode == "def" else M.config(M.RICH, M.ATK)
    hp = M.hyper(multi)
    (seed,), (env,) = M.ok_seeds(L, 1, 0, omode, multi=multi, cfg=cfg, hp=hp)
    acted = {"def": 0, "atk": 0, "idle": 0}
    for k in range(100):
        dm, _, am = reference_masks(M.oracle_state(env), L, cfg, hp, mode, multi, cap=False)
        d, a, dn, an = S.reference_sample(dm, am, 77, k, 0, 0.3, 0.3, L, multi)
        kw = {}
        if mode != "atk":
            kw["def_act"] = d
        if mode != "def":
            kw["atk_act"] = a
        _, _, done, info = env.step(**kw)
        real, fc = info["RealAction"], info["FailCode"]
        if mode == "def" and multi:
            assert np.array_equal(real, d), k
            acted["def"] += int(d.any())
        elif mode == "def":
            assert real == d and (d == A or fc == 0), (k, d, real, fc)
            acted["def"] += int(d != A)
            acted["idle"] += int(d == A and dn > 0)
        elif mode == "atk":
            rt = U.atk_pick(a)
            assert rt is None or _summoned(fc, real, rt), (k, rt, fc)
            acted["atk"] += int(rt is not None)
        else:  # TDMulti: a defender that acted replaces the whole RealAction dict (TDMulti.py:114)
            rt = U.atk_pick(a)
            if d != A:
                assert real == d and fc["Defender"] == 0, (k, d, real, fc)
                acted["def"] += 1
            else:
                assert real["Defender"] == A
            assert rt is None or (len(fc["Attacker"]) > rt[0] and fc["Attacker"][rt[0]] == 0), (k, rt, fc)
            acted["atk"] += int(rt is not None)
        if done:
            M.reset_ok(env)
    assert mode == "atk" or acted["def"] > 5, acted
    assert mode == "def" or acted["atk"] > 5, acted
