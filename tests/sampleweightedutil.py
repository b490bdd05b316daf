"""Shared pieces of the weighted-sampling tests (tests/test_gpu_sample_weighted.py on the device,
scripts/sample_weighted_seed_search.py on the CPU oracle): the weight patterns of the
sampler-driven run and the reference over a whole batch.  Not a test module."""
import numpy as np

from gym_TD import sampling as S
from gym_TD.masks import reference_masks

PATTERNS = ("uniform", "sparse", "boost", "ones")


def pattern_of(step):
    """The pattern of a step: all four in turn, and all four among the steps k % 10 == 0 too
    (k = 0, 10, 20, 30 give 0, 3, 2, 1)."""
    return PATTERNS[(step + step // 10) % 4]


def run_weights(step, B, L, mode):
    """(def_w, atk_w) float32 (B, 6 L^2 + 1) / (B, 13) of a step of the run, None for a side the
    mode lacks: a fresh array seeded by the step.
      uniform  U(0, 1)
      sparse   U(0, 1) with 95 % of the entries zero
      boost    U(0, 1); builds x 2^-6 and the no-op x 2^-3 (level-up and destruct x 1), so that a
               board of thousands of build entries reaches its level-ups; attacker: "nothing" x 2^-3
      ones     all 1, the always-legal entry 0"""
    rng = np.random.RandomState(1000 + step)
    NC, p = L * L, pattern_of(step)
    out = []
    for n, want in ((6 * NC + 1, mode != "atk"), (13, mode != "def")):
        w = rng.rand(B, n).astype(np.float32)
        if p == "sparse":
            w *= rng.rand(B, n) < 0.05
        elif p == "boost":
            if n != 13:
                w[:, :4 * NC] *= np.float32(2.0 ** -6)
            w[:, -1] *= np.float32(2.0 ** -3)
        elif p == "ones":
            w[:] = 1.0
            w[:, -1] = 0.0
        out.append(w if want else None)
    return out


def reference_batch_weighted(states, L, cfg, hp, mode, seed, ticket, def_w, atk_w, boards=None):
    """reference_sample_weighted over reference_masks of states[b] for every board id b in
    ``boards`` (default: all): {b: (def_act, atk_act, def_mass, atk_mass)}."""
    out = {}
    for b in (range(len(states)) if boards is None else boards):
        dm, _, am = reference_masks(states[b], L, cfg, hp, mode, False)
        out[b] = S.reference_sample_weighted(dm, am, None if def_w is None else def_w[b],
                                             None if atk_w is None else atk_w[b], seed, ticket, b, L)
    return out
