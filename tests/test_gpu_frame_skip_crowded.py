"""Frame skip on the crowded and full boards of tests/test_gpu_crowded.py.

skip_board (td_step_skip.h) keeps a board's enemy and tower lists in LDS across the k
sub-steps of a macro step and stores them once: the sort and the compaction across the
list's halves run k times on one LDS image, TD-atk swaps raw and packed cell words around
its built-in defender, and the flags are ORed over the loop.  The recipe of
tests/test_gpu_frame_skip.py never brings a board past 64 enemies, to a full tower list or
to a cap refusal; the scenarios of tests/crowdutil.py do, and crowdutil.Reference(scn, k)
restates them at frame skip k: the policy's actions once per macro step, the empty actions
in between, the oracle's counters over every sub-step.

Every case asserts the scenario's floors on those counters first (the same ones at the same
k without a GPU in tests/test_crowded_ref.py), then compares at every macro step and for every
board still running what tests/test_gpu_crowded.py compares at every step, bit for bit, and
the flag words at the end.
"""
import pytest
import torch

import crowdutil as U

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

import test_gpu_crowded as G  # noqa: E402  (the engine, the per-board comparison)


@pytest.mark.parametrize("name,k", U.SKIP_CASES)
def test_crowded_boards_at_frame_skip(name, k):
    scn = U.BY_NAME[name]
    ref = U.reference(scn, k)
    print(name, k, ref.counters, ref.refused)
    U.check_scenario(ref)
    eng = G._engine(scn, ref.seeds, "large")
    try:
        eng.set_frame_skip(k)
        assert "td_skip_kernel" in eng.step_kernel_name
        _, failed = eng.reset()
        assert not failed
        compared = 0
        for i, (da, aa, want) in enumerate(ref.steps):
            G._step(eng, da, aa)
            out = G._Out(eng)
            for b, w in enumerate(want):
                if w is not None:  # (else: finished in an earlier macro step, no auto-reset here)
                    G._check_board(scn, eng, out, b, w, (name, k, i, b))
                    compared += 1
        assert len(ref.steps) == scn.steps // k and compared >= (scn.B - 1) * len(ref.steps)
        assert eng.flags().tolist() == ref.flags(), (eng.flags().tolist(), ref.refused)
        if not scn.capped:
            assert (eng.flags() == 0).all()
    finally:
        eng.close()
