"""Shared pieces of the action-sampling tests (tests/test_sample_ref.py on the CPU,
tests/test_gpu_sample_actions.py on the device): the known answers of the random word, the
reference over a whole batch, and what "the step executed the sampled action" means per mode.
Not a test module."""
import numpy as np

from gym_TD import sampling as S
from gym_TD.masks import reference_masks

# (seed, ticket, board, draw) -> (word, u): td_sample.h's rule, computed independently
KNOWN = [
    ((0, 0, 0, 0), 0x238275BC38FCBE91, 595752380),
    ((0, 0, 0, 1), 0x421DAF3033E887A3, 1109241648),
    ((1, 2, 3, 1), 0xB39B489899B5598A, 3013298328),
    ((0xDEADBEEFCAFEF00D, 2 ** 64 - 1, 65535, 3), 0x72FF560395D91BD3, 1929336323),
    ((2026, 7, 2099, 2), 0x7904480F124E732B, 2030323727),
]
SM0 = 0xE220A8397B1DCDAF  # splitmix64's published first output for state 0

IDLE_03 = 0x4CCCCCCC  # 0.3 in units of 2^-32, as min(2**32 - 1, int(0.3 * 2**32)) gives it


def chi2(counts):
    counts = np.asarray(counts, dtype=np.float64)
    e = counts.sum() / len(counts)
    return float(((counts - e) ** 2 / e).sum())


def reference_batch(states, L, cfg, hp, mode, multi, seed, ticket, def_idle, atk_idle, boards=None):
    """reference_sample over reference_masks of states[b] for every board id b in ``boards``
    (default: all): {b: (def_act, atk_act, def_count, atk_count)}."""
    out = {}
    for b in (range(len(states)) if boards is None else boards):
        dm, _, am = reference_masks(states[b], L, cfg, hp, mode, multi)
        out[b] = S.reference_sample(dm, am, seed, ticket, b, def_idle, atk_idle, L, multi)
    return out


def atk_pick(atk_act):
    """(road, type) of a sampled attacker action (3, 8), or None: the sampler sets one first slot at most."""
    a = np.asarray(atk_act)
    assert a.shape == (3, 8) and (a[:, 1:] == 4).all() and (a[:, 0] != 4).sum() <= 1, a
    roads = np.flatnonzero(a[:, 0] != 4)
    return (int(roads[0]), int(a[roads[0], 0])) if len(roads) else None
