"""bench.py's plain run and ``--dump-outputs`` on a small batch.

A plain run (no ``--full``) prints the one JSON line with ``ms_per_step`` for the ``--steps``
it was given and no CPU-baseline leg.  Two runs with the same arguments write the same
arrays, byte for byte: obs / reward / done and the info arrays of the last timed step, as
float32 / float64 ``.npy`` files, here all boards of each (1,024 boards fit every share)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K = 1024, 7


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--global-batch", str(B),
                               "--steps", str(K), "--warmup", "2", "--burnin", "150", "--dump-outputs", d],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for d in dirs]
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, so[-2000:] + se[-4000:]
        lines = [ln for ln in so.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, so[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == K and d["ms_per_step"] > 0 and d["unit"] == "env-steps/s" and d["dtype"] == "f64"
        assert d["value"] == pytest.approx(B * K / (d["ms_per_step"] * K / 1e3), rel=1e-9)
        assert d["higher_is_better"] is True and d["board_flags_nonzero"] == 0
        assert "cpu_baseline" not in d and "cpu_baseline_python" not in d  # --full's legs
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"obs.npy", "reward.npy", "done.npy", "win.npy", "ep_return.npy", "ep_len.npy", "real_def.npy",
            "fail_def.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n))
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == B, n
        assert a.tobytes() == b.tobytes(), n
        total += a.nbytes
    assert total <= 64 * 10 ** 6
    obs, reward = np.load(os.path.join(dirs[0], "obs.npy")), np.load(os.path.join(dirs[0], "reward.npy"))
    assert obs.shape == (B, 45, 10, 10) and obs.dtype == np.float32 and reward.dtype == np.float64
    assert np.isfinite(obs).all() and obs.any() and np.isfinite(reward).all()
