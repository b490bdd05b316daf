"""`steps >= upgrade_step` stands for `steps / max_episode_steps >= enemy_upgrade_at` in the step
kernels (gym-td_amd/csrc/td_upgrade_step.h, summon_cluster) without a GPU:
scripts/upgrade_step_host.cpp compares the two for every episode limit and threshold of its
lists -- every s in [0, limit + 2], s = 2^31 - 1 and 1,000 random s each -- as a stand-alone host
program under the address and undefined-behaviour sanitizers; and the values it computes are
compared here with Python's own division (the oracle's: td_oracle.py Board.step,
summon_cluster), over the same step counts."""
import random
import subprocess

import numpy as np

from test_capi_tables_host import _run, cxx  # noqa: F401  (the compiler fixture and the runner)

LIMITS = (1, 2, 3, 7, 1200, 4095, 4096, 10 ** 6)
INT32_MAX = 2 ** 31 - 1


def _thresholds(limit, rng):
    out = [-1.0, 0.0, 0.75, 1.0, 1.0 + 2.0 ** -52, 2.0, 1.0 / 3.0]
    for s in [0, 1, limit - 1, limit, limit + 1, limit + 2] + [rng.randrange(limit + 3) for _ in range(6)]:
        q = s / limit
        out += [q, float(np.nextafter(q, -np.inf)), float(np.nextafter(q, np.inf))]
    return out


def test_upgrade_step_under_sanitizers(cxx, tmp_path):  # noqa: F811
    out = _run(cxx, tmp_path, "upgrade_step")
    # 8 limits x 43 thresholds x (limit + 3 counts, 2^31 - 1, 1,000 random)
    assert int(out.split("upgrade_step: ")[1].split()[0]) >= 8 * 43 * 1001


def test_upgrade_step_equals_pythons_division(cxx, tmp_path):  # noqa: F811
    _run(cxx, tmp_path, "upgrade_step")  # (builds the program)
    exe = str(tmp_path / "upgrade_step_host")
    rng = random.Random(7)
    pairs = [(limit, t) for limit in LIMITS for t in _thresholds(limit, rng)]
    args = [a for limit, t in pairs for a in (str(limit), float(t).hex())]
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [int(v) for v in run.stdout.split()]
    assert len(got) == len(pairs)
    nrng = np.random.RandomState(3)
    for (limit, t), us in zip(pairs, got):
        s = np.concatenate([np.arange(0, limit + 3, dtype=np.int64), [INT32_MAX],
                            nrng.randint(0, 2 ** 31, size=1000, dtype=np.int64)])
        by_division = s.astype(np.float64) / np.float64(limit) >= t
        bad = np.flatnonzero(by_division != (s >= us))
        assert bad.size == 0, (limit, float(t).hex(), us, s[bad[:5]].tolist())
        # the smallest such count, 0 for a threshold <= 0
        assert us == 0 if t <= 0 else (us > 0 and not (us - 1) / limit >= t and us / limit >= t), (limit, t, us)
