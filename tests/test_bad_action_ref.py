"""The out-of-range-action runs on the CPU oracles alone (tests/badact.py, no GPU).

tests/test_gpu_bad_action.py compares the device with these runs bit for bit.  Its pass says
that a step kernel reads all 64 bits of an action only if the runs do send values whose low
word alone is a legal action that would change the board: asserted here, as a condition and
not a measurement, on copies of the oracle -- at least 8 such "live" 2^32 + a values per case,
each of which gives another state digest when ``a`` is stepped in its place.  Likewise: at
least 4 bad values sent to a side that is cooling down, every kind of value, boards flagged
late, a flag carried across an auto-reset, a flag set in the very step that auto-resets, in
TD-2p both sides bad in one step, and at frame skip 3 a bad value's macro step ending the
episode at each of the sub-steps 0, 1 and 2.
"""
import numpy as np
import pytest

import badact as A

CASES = [c + (1,) for c in A.DISCRETE + A.MULTI] + [c + (A.SKIP_K,) for c in A.SKIP]


def test_sanitise_is_the_documented_rule():
    L = 10
    for v in (-1, -2 ** 63, 2 ** 31, 601, A.HI + 17):
        assert A.sanitise(L, v) == (600, None, True)
    for v in (0, 17, 599, 600):
        assert A.sanitise(L, v) == (v, None, False)
    a = np.full((3, 8), 4, dtype=np.int64)
    a[1] = [0, 5, 3, -1, A.HI + 2, 2 ** 31, -2 ** 63, 4]
    _, sa, bad = A.sanitise(L, None, a)
    assert bad and sa[1].tolist() == [0, 4, 3, 4, 4, 4, 4, 4] and (sa[[0, 2]] == 4).all()
    assert not A.sanitise(L, None, sa)[2]
    m = np.zeros((6, L, L), dtype=np.int64)
    m[0, 0, :6] = [1, 2, 3, -1, A.HI + 1, 2 ** 31]
    sm, _, bad = A.sanitise(L, m, None, multi=True)
    assert bad and sm[0, 0, :6].tolist() == [1, 2, 0, 0, 0, 0] and sm.sum() == 3
    assert not A.sanitise(L, sm, None, multi=True)[2]


@pytest.mark.parametrize("mode,multi,L,k", CASES)
def test_run_reaches_what_it_is_there_for(mode, multi, L, k):
    tr = A.Trace(mode, L, multi, k)
    print(mode, multi, L, k, "live", tr.live, "cooling", tr.cool, tr.kinds, "ends with a bad value", tr.ends_bad,
          "both", tr.both, "flagged resets", tr.resets_flagged)
    A.check_trace(tr)
    # the values as sent: int64, out of range exactly where the expected flags rise
    d, a = tr.acts[0]
    assert (d is None or d.dtype == np.int64) and (a is None or a.dtype == np.int64)
    seen = np.zeros(A.B, dtype=bool)
    for s, (d, a) in enumerate(tr.acts):
        for b in range(A.B):
            seen[b] |= A.sanitise(L, None if d is None else (d[b] if multi else int(d[b])),
                                  None if a is None else a[b], multi)[2]
        assert ((tr.flags[s] != 0) == seen).all(), s
