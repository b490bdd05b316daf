"""The rule of td_sample_weighted on the CPU (no GPU): gym_TD.sampling's quantiser at its edges,
the threshold and the pick against answers computed here in plain Python ints, hand-made rows
(illegal entries, S == 0, one-hot), the distribution of the picks, weights_from_logits, and the
same rule as C++ (csrc/td_sample.h, with td_call_check.h's io check) run as a stand-alone program
under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sampleutil as U
from gym_TD import sampling as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
L = 10
A = 6 * L * L
Q1 = 2 ** 31
M64 = 2 ** 64 - 1


def _f32(bits):
    return np.frombuffer(struct.pack("<I", bits), dtype=np.float32)[0]


def _bits(x):
    return struct.unpack("<I", np.float32(x).tobytes())[0]


BELOW_1 = np.nextafter(np.float32(1), np.float32(0))
BELOW_2M31 = np.nextafter(np.float32(2.0 ** -31), np.float32(0))
# (weight, q): the quantiser's table
EDGES = [
    (np.float32(0.0), 0), (np.float32(-0.0), 0), (np.float32(-1.0), 0), (np.float32("nan"), 0),
    (np.float32("inf"), Q1), (np.float32(2.0), Q1), (np.float32(1.0), Q1), (BELOW_1, Q1 - 128),
    (np.float32(2.0 ** -31), 1), (BELOW_2M31, 0), (_f32(0x00000400), 0),  # a subnormal
    (np.float32("-inf"), 0), (np.float32(0.5), 2 ** 30), (np.float32(0.3), 644245120), (np.float32(3 * 2.0 ** -31), 3),
]


# ---------------------------------------------------------------------------- the quantiser
def test_quantiser_edges():
    for w, q in EDGES:
        assert int(S.quantize(w)) == q, (w, q)
    got = S.quantize(np.array([w for w, _ in EDGES], dtype=np.float32))
    assert got.dtype == np.int64 and got.tolist() == [q for _, q in EDGES]
    # independent of the float path: the value from the bits (exponent and mantissa) for random floats in (0, 1)
    rng = np.random.RandomState(3)
    for bits in rng.randint(0x2F000000, 0x3F800000, size=2000):
        e, mant = int(bits) >> 23, (int(bits) & 0x7FFFFF) | 0x800000
        sh = e - 119  # mant * 2^(e - 150) * 2^31
        want = mant << sh if sh >= 0 else mant >> -sh
        assert int(S.quantize(_f32(int(bits)))) == want, hex(bits)
    assert S.quantize(np.float64(0.3)) == 644245120  # taken as float32 first


def test_weights_from_logits():
    rng = np.random.RandomState(1)
    x = (rng.randn(5, 601) * 30).astype(np.float32)
    w = S.weights_from_logits(x)
    assert w.dtype == np.float32 and w.shape == x.shape
    assert (w.max(axis=1) == 1.0).all() and (w >= 0).all()
    assert np.array_equal(w, np.exp(x - x.max(axis=1, keepdims=True)).astype(np.float32))
    assert (S.quantize(w).max(axis=1) == Q1).all()
    torch = pytest.importorskip("torch")
    t = S.weights_from_logits(torch.from_numpy(x))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and (t.max(dim=1).values == 1.0).all()
    assert np.allclose(t.numpy(), w, rtol=1e-5, atol=1e-37)  # (two exp implementations: a few ulp, more among subnormals)
    assert S.weights_from_logits(torch.from_numpy(x).double()).dtype == torch.float32


# ------------------------------------------------------------------------- known answers
def _by_hand(m, w64):
    """The rule in plain ints, written apart from gym_TD.sampling: (pick, m, S)."""
    total = 0
    for x in m:
        total += x
    if total == 0:
        return len(m) - 1, 0, 0
    r = (w64 * total) // 2 ** 64
    run = 0
    for e in range(len(m)):
        run = run + m[e]
        if run > r:
            return e, m[e], total
    raise AssertionError


ROW_A = [3, 0, 5, Q1, 1]  # S = 2^31 + 9
# (row, word, pick, m, S): scripts/sample_weighted_rule_host.cpp holds the same
KNOWN = [
    (ROW_A, 0, 0, 3, Q1 + 9),
    (ROW_A, M64, 4, 1, Q1 + 9),
    (ROW_A, 1 << 63, 3, Q1, Q1 + 9),
    (ROW_A, 0xEFFFFFFF, 0, 3, Q1 + 9),
    (ROW_A, 0x600000000, 2, 5, Q1 + 9),
    ([0, 0, 0], 0x123456789ABCDEF, 2, 0, 0),
    ([0, 0, 77, 0], M64, 2, 77, 77),
    ([0, 0, 0, 9], 1 << 62, 3, 9, 9),
    ([Q1] * 6145, M64, 6144, Q1, 6145 << 31),
    ([Q1] * 6145, 1 << 63, 3072, Q1, 6145 << 31),
    ([Q1] * 8192, M64, 8191, Q1, 1 << 44),  # S = 2^44 with the word 2^64 - 1: r = 2^44 - 1
    ([Q1] * 8192, M64 - (1 << 20), 8191, Q1, 1 << 44),
    ([Q1] * 8192, 0xFFF0000000000000, 8190, Q1, 1 << 44),
]


def test_known_answers():
    for row, w64, pick, m, tot in KNOWN:
        assert _by_hand(row, w64) == (pick, m, tot), (row[:5], hex(w64))
        assert S.pick_weighted(row, w64) == (pick, (m, tot)), (row[:5], hex(w64))
    rng = np.random.RandomState(8)
    for _ in range(300):
        n = int(rng.randint(1, 40))
        row = [int(x) for x in rng.randint(0, Q1 + 1, size=n) * (rng.rand(n) < 0.5)]
        w64 = (int(rng.randint(0, 2 ** 32)) << 32) | int(rng.randint(0, 2 ** 32))
        p, m, tot = _by_hand(row, w64)
        assert S.pick_weighted(row, w64) == (p, (m, tot))
        assert tot == 0 or row[p] > 0


# -------------------------------------------------------------------------- hand-made rows
def _def_mask(legal):
    m = np.zeros(A + 1, dtype=np.uint8)
    m[list(legal)] = 1
    m[A] = 1
    return m


def _weights(pairs, fill=0.0):
    w = np.full(A + 1, fill, dtype=np.float32)
    for a, x in pairs:
        w[a] = x
    return w


def _sw(dm, am, dw, aw, b=0, ticket=0, seed=9):
    return S.reference_sample_weighted(dm, am, dw, aw, seed, ticket, b, L)


def test_reference_uses_draws_1_and_3_with_the_whole_word():
    dm, dw = _def_mask(range(0, A, 3)), np.random.RandomState(0).rand(A + 1).astype(np.float32)
    am = np.ones((3, 5), dtype=np.uint8)
    aw = np.random.RandomState(1).rand(13).astype(np.float32)
    for b in range(40):
        d, a, dmass, amass = _sw(dm, am, dw, aw, b=b, ticket=5)
        m = [int(x) if dm[i] else 0 for i, x in enumerate(S.quantize(dw))]
        assert (d, dmass[0], dmass[1]) == _by_hand(m, S.word(9, 5, b, 1))
        e, me, tot = _by_hand([int(x) for x in S.quantize(aw)], S.word(9, 5, b, 3))
        assert amass == (me, tot) and a.shape == (3, 8) and a.dtype == np.int64
        assert U.atk_pick(a) == (None if e == 12 else (e // 4, e % 4))


def test_an_illegal_entry_with_weight_one_never_wins():
    dm = _def_mask([7, 300])
    dw = _weights([(7, 2.0 ** -20), (300, 2.0 ** -20), (A, 2.0 ** -20)], fill=1.0)  # every illegal entry: weight 1
    dw[[7, 300, A]] = np.float32(2.0 ** -20)
    seen = set()
    for t in range(300):
        d, _, mass, _ = _sw(dm, None, dw, None, ticket=t)
        assert d in (7, 300, A) and mass == (2 ** 11, 3 * 2 ** 11)
        seen.add(d)
    assert seen == {7, 300, A}
    am = np.zeros((3, 5), dtype=np.uint8)
    am[:, 4] = 1
    am[1, 2] = 1
    aw = np.ones(13, dtype=np.float32)
    for t in range(100):
        _, a, _, mass = _sw(None, am, None, aw, ticket=t)
        assert U.atk_pick(a) in (None, (1, 2)) and mass == (Q1, 2 * Q1)


def test_zero_total_is_the_noop_with_mass_zero():
    for dw in (_weights([]), _weights([(5, 1.0)]), _weights([(3, -1.0), (A, np.float32("nan"))])):
        for b in range(20):
            d, a, dmass, amass = _sw(_def_mask([3]), None, dw, None, b=b)
            assert d == A and dmass == (0, 0) and a is None and amass is None
    am = np.ones((3, 5), dtype=np.uint8)
    _, a, _, amass = _sw(None, am, None, np.zeros(13, dtype=np.float32))
    assert (a == 4).all() and amass == (0, 0)
    # a closed cool-down: reference_masks leaves the no-op alone, so only its weight counts
    d, _, mass, _ = _sw(_def_mask([]), None, _weights([(A, 0.25)], fill=1.0), None)
    assert d == A and mass == (2 ** 29, 2 ** 29)


def test_one_hot_legal_row_at_every_ticket():
    for k in (0, 299, A - 1, A):
        dw = _weights([(k, 0.125)])
        for t in range(200):
            d, _, mass, _ = _sw(_def_mask(range(A)), None, dw, None, ticket=t, b=t % 7)
            assert d == k and mass == (2 ** 28, 2 ** 28), (k, t)
    am = np.ones((3, 5), dtype=np.uint8)
    for e in (0, 11, 12):
        aw = np.zeros(13, dtype=np.float32)
        aw[e] = 1.0
        for t in range(50):
            _, a, _, mass = _sw(None, am, None, aw, ticket=t)
            assert U.atk_pick(a) == (None if e == 12 else (e // 4, e % 4)) and mass == (Q1, Q1)


def test_quantiser_table_scattered_over_legal_entries():
    legal = list(range(10, 10 + len(EDGES)))
    dw = _weights([(a, w) for a, (w, _) in zip(legal, EDGES)])
    total = sum(q for _, q in EDGES)
    for t in range(100):
        d, _, mass, _ = _sw(_def_mask(legal), None, dw, None, ticket=t)
        assert mass[1] == total and mass[0] == dict(zip(legal, (q for _, q in EDGES)))[d] > 0


# ---------------------------------------------------------------------------- distribution
def test_picks_follow_the_weights():
    """20,000 tickets on one row of five legal entries with weights 1, 1/2, 1/4, 1/8, 1/8 (seed
    12345, board 0): chi^2 against m / S below 18.47, the 0.999 quantile of 4 degrees of freedom
    (deterministic: the value is printed)."""
    legal = [2, 100, 250, 431, A]
    wts = [1.0, 0.5, 0.25, 0.125, 0.125]
    dm, dw = _def_mask(legal[:-1]), _weights(list(zip(legal, wts)), fill=0.0)
    dw[[0, 1, 599]] = 1.0  # illegal
    counts = dict.fromkeys(legal, 0)
    n = 20000
    for t in range(n):
        d, _, mass, _ = _sw(dm, None, dw, None, seed=12345, ticket=t)
        counts[d] += 1
        assert mass[1] == 2 * Q1
    exp = np.array(wts) / 2.0 * n
    got = np.array([counts[a] for a in legal], dtype=np.float64)
    x = float(((got - exp) ** 2 / exp).sum())
    print("chi2 weighted: %.2f" % x, counts)
    assert x < 18.47, x


# ------------------------------------------------------------------ the rule as a host program
def test_rule_as_a_host_program_under_sanitizers(tmp_path):
    """scripts/sample_weighted_rule_host.cpp: the quantiser's edges, the threshold, the known
    answers and the io check's verdicts with their whole messages, in refusal order; then the
    program's answers for the table above and for random rows against the Python mirror."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + FLAGS + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "sample_weighted_rule_host")
    cc = subprocess.run([cxx] + FLAGS + ["-o", exe, os.path.join(ROOT, "scripts", "sample_weighted_rule_host.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.search(r"^sample_weighted_rule: \d+ cases ok$", run.stdout, re.M), run.stdout
    for w, q in EDGES:
        out = subprocess.run([exe, "q", hex(_bits(w))], capture_output=True, text=True)
        assert out.returncode == 0 and int(out.stdout) == q, (w, out.stdout, out.stderr)
    rng = np.random.RandomState(5)
    rows = [(row, w64) for row, w64, _, _, _ in KNOWN if len(row) < 100]
    for _ in range(8):
        n = int(rng.randint(1, 30))
        rows.append(([int(x) for x in rng.randint(0, Q1 + 1, size=n)],
                     (int(rng.randint(0, 2 ** 32)) << 32) | int(rng.randint(0, 2 ** 32))))
    for row, w64 in rows:
        out = subprocess.run([exe, hex(w64)] + [str(x) for x in row], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert tuple(int(x) for x in out.stdout.split()) == _by_hand(row, w64), (row, hex(w64))
