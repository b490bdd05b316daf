"""Driving an engine on a caller's stream that lags behind the host, and comparing it with a
twin driven on the default stream: the shared pieces of tests/test_gpu_streams.py.  Not a test
module.

The default stream of the suite is the legacy NULL stream.  With ``stream == NULL`` the step
stream and the NULL stream are one queue, so work enqueued on the wrong one, or a NULL-stream
runtime call in front of a launch on the step stream, is in order by construction.  On a
non-blocking stream that still has a spin queued while the host issues the next calls it is not.
"""
import numpy as np
import torch

from gym_TD import _lib

# torch.cuda._sleep(SPIN_CYCLES): see lag()
SPIN_CYCLES = 3600000

OUTPUTS = ("obs", "reward", "done", "win", "allow_next", "cooldowns", "ep_return", "ep_len", "real_def", "fail_def",
           "real_atk", "fail_atk")
SUM = "stats.sum (atomic adds)"


def lag(stream, cycles=SPIN_CYCLES):
    """Enqueue a spin on ``stream`` (torch.cuda._sleep): what is enqueued behind it waits.

    Measured on an MI355X with a pair of torch events around one spin on a pool stream:
    1,000,000 cycles 0.420 ms, 3,000,000 cycles 1.254 ms, 10,000,000 cycles 4.171 ms (twice each,
    equal to 1 us), so 0.417 us per 1,000 cycles and SPIN_CYCLES = 3,600,000 cycles about 1.5 ms:
    several times what the host needs to issue a group of ten calls.  A test enqueues at most a
    few hundred spins, well below one second in all."""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(cycles))


def ran_ahead(stream):
    """True if ``stream`` still has work queued now: the host finished issuing the calls in front
    of this one while the stream had not finished them.  It shows that the host ran ahead of the
    stream; it does not show which hardware queue the stream got."""
    ev = torch.cuda.Event()
    ev.record(stream)
    return not ev.query()


def _rows(a, B):
    return np.ascontiguousarray(a).view(np.uint8).reshape(B, -1)


def snapshot(eng, extra=None):
    """Everything compared between twins, as uint8 arrays [B, bytes] by field name: every output
    tensor, the exported state (enemy / tower slots at or past n_en / n_tw zeroed), both RNG
    streams of every board, the flags, the episode records, the episode count -- and the f64 sum
    of returns as a float (sum_tolerance).  ``extra``: further named tensors or arrays with one
    row per board (masks, status words, ...), compared as bytes too.  Reads on torch's current
    stream; waits for the device."""
    B = eng.B
    s = {}
    for n in OUTPUTS:
        t = getattr(eng, n)
        if t is not None:
            s["out." + n] = _rows(t.view(torch.uint8).cpu().numpy(), B)
    st = {k: v.copy() for k, v in eng.export_state().items()}
    for names, n, cap in ((("en_lp", "en_mg", "en_inf"), st["hdr"]["n_en"], _lib.ECAP),
                          (("tw_cd", "tw_inf"), st["hdr"]["n_tw"], _lib.TCAP)):
        dead = np.arange(cap)[None, :] >= n[:, None]
        for name in names:
            st[name][dead] = 0
    for k, v in st.items():
        s["state." + k] = _rows(v, B)
    s["flags"] = _rows(eng.flags(), B)
    s["np"] = _rows(np.stack([eng.get_np_state(b) for b in range(B)]), B)
    s["py"] = _rows(np.stack([np.asarray(eng.get_py_state(b)) for b in range(B)]), B)
    for k, t in zip(("ret", "len", "win"), eng.episode_records()):
        s["rec." + k] = _rows(t.cpu().numpy(), B)
    stats = eng.episode_stats().cpu().numpy()
    s["stats.n"] = _rows(stats[:1], 1)
    s[SUM] = float(stats[1])
    for k, v in (extra or {}).items():
        v = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        s["extra." + k] = _rows(v, v.shape[0] if v.ndim else 1)
    return s


def sum_tolerance(n):
    """tests/test_gpu_board_lists_dev.py's rule for the one field compared with a tolerance:
    td_episode_stats' sum is accumulated with atomic adds in the order the waves arrive; two
    orders of summing n terms differ by at most 2 (n - 1) u sum|x_i|, u = 2^-53, |x_i| < 1.6e4."""
    return 2.0 * max(n - 1, 0) * 2.0 ** -53 * n * 1.6e4


def episodes(snap):
    """The count of finished episodes in a snapshot."""
    return int(snap["stats.n"].view(np.float64)[0, 0])


NP_LEAD_DRAWS = 1 << 16


def _np_outputs(state, n):
    """The next n 32-bit outputs of a layout stream given as get_np_state()'s bytes."""
    w = np.ascontiguousarray(state).view(np.uint32)
    r = np.random.RandomState()
    r.set_state(("MT19937", w[:624], int(w[624])))
    return np.frombuffer(r.bytes(4 * n), dtype=np.uint32)


def same_np_stream(x, y):
    """True if one of the two layout streams is the other advanced by fewer than NP_LEAD_DRAWS
    draws: the next 64 outputs of one are found among the next outputs of the other."""
    for p, q in ((x, y), (y, x)):
        far, near = _np_outputs(p, NP_LEAD_DRAWS + 64), _np_outputs(q, 64)
        for d in np.flatnonzero(far[:NP_LEAD_DRAWS] == near[0]):
            if np.array_equal(far[d:d + 64], near):
                return True
    return False


def same(a, b, where, np_lead=False):
    """Assert that snapshot ``a`` equals snapshot ``b``, naming the first board and field that differ.

    np_lead: the engines stage layouts ahead of play with refills on their side streams
    (auto-reset, random_agent=True, a refill interval > 0).  A refill reads a ring's head while
    the step beside it may be advancing it (td_reset.hip td_refill_kernel), so how far a board's
    layout stream has been drawn AHEAD at a given moment depends on timing; which layouts it
    yields, in which order, does not.  There a board's layout stream must be the twin's stream --
    the same outputs to come -- at a lead of fewer than NP_LEAD_DRAWS draws either way
    (same_np_stream); everywhere else, and for every other field, byte for byte."""
    assert set(a) == set(b), (where, sorted(set(a) ^ set(b)))
    for k in sorted(b):
        if k == SUM:
            continue
        assert a[k].shape == b[k].shape, (where, k, a[k].shape, b[k].shape)
        if k == "np" and np_lead:
            for board in np.flatnonzero((a[k] != b[k]).any(axis=1)):
                assert same_np_stream(a[k][board], b[k][board]), \
                    "%s: board %d's layout stream is not the twin's at another lead" % (where, board)
            continue
        if not np.array_equal(a[k], b[k]):
            rows = np.flatnonzero((a[k] != b[k]).any(axis=1))
            byte = int(np.flatnonzero(a[k][rows[0]] != b[k][rows[0]])[0])
            raise AssertionError("%s: field %s differs, first at board %d (byte %d: %d, twin %d); %d board(s) differ"
                                 % (where, k, rows[0], byte, a[k][rows[0], byte], b[k][rows[0], byte], len(rows)))
    n = episodes(b)
    assert abs(a[SUM] - b[SUM]) <= sum_tolerance(n), (where, SUM, a[SUM], b[SUM], n)
