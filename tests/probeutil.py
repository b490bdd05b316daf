"""Shared pieces of tests/test_gpu_probe.py: engines with a replayable call history, the twins a
probe is defined by, and the byte-for-byte comparisons.  Not a test module.

The twin for replica r is a fresh engine with the same seeds and the same call history, on which
``playout(steps, boards, ticket + r * steps)`` is run: what the probe's replica must equal, output
for output.  Everything "expected" here comes from the twins, never from the probe."""
import numpy as np
import torch

import streamutil as SU
from gym_TD import sampling as S
from gym_TD.engine import TDEngine
from test_gpu_action_mask import _engine
from test_gpu_playout import SEED, _drive

PROBE_OUT = ("reward", "done", "steps_run", "win", "first_def", "first_atk")
POISON = 0xA5


def engine(L, B, mode, cfg, hp, autoreset, history=None, seed0=500, **kw):
    """An engine on seeds seed0 .. seed0 + B - 1, reset, with ``history(eng)`` replayed on it."""
    if kw:
        seeds = np.arange(B) + seed0
        eng = TDEngine(L, B, mode, False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=autoreset, cfg=cfg, hp=hp, **kw)
        eng.reset_all()
    else:
        eng = _engine(L, B, mode, False, cfg, hp, autoreset, seed0)
    eng.sample_seed = SEED
    if history is not None:
        history(eng)
    return eng


def spread(limit, stride=4):
    """A history: board b is stepped to limit - 1 - stride * (b mod 12) steps of its episode, so a
    probe of a few sub-steps ends some boards' episodes at the step limit and leaves others open."""
    def history(eng):
        pre = np.maximum(limit - 1 - stride * (np.arange(eng.B) % 12), 0)
        for p in range(int(pre.max())):
            _drive((eng,), np.flatnonzero(pre > p), 5000 + p)
    return history


def full_steps(n, ticket0=7000):
    """A history of n ordinary steps of every board with sampled actions."""
    def history(eng):
        for t in range(n):
            out = eng.sample_actions(ticket=ticket0 + t, def_idle=0.3, atk_idle=0.3)
            eng.step(def_act=out["def"], atk_act=out["atk"])
    return history


def host(out):
    return {n: v.cpu().numpy().copy() for n, v in out.items() if v is not None}


def twins(make, steps, reps, boards, ticket, di=0.0, ai=0.0, hook=None):
    """The replicas' outputs by definition: {name: array [B][reps]...} over fresh engines
    ``make()``, replica r from ``playout(steps, boards, ticket + r * steps, first=True)``.
    hook(r, eng, when): optional, called with when = "before" and "after" each twin's playout."""
    want = None
    for r in range(reps):
        eng = make()
        try:
            if hook is not None:
                hook(r, eng, "before")
            got = host(eng.playout(steps, boards, ticket=(ticket + r * steps) & S.M64, def_idle=di, atk_idle=ai, first=True))
            if hook is not None:
                hook(r, eng, "after")
        finally:
            eng.close()
        if want is None:
            want = {n: np.zeros((v.shape[0], reps) + v.shape[1:], dtype=v.dtype) for n, v in got.items() if n in PROBE_OUT}
        for n in want:
            want[n][:, r] = got[n]
    return want


def same_rows(got, want, rows, where):
    """The probe's rows (a dict of device tensors or None) of the named boards against the
    twins', bit for bit."""
    got = host(got)
    assert set(got) == set(want), (where, sorted(got), sorted(want))
    for n in want:
        g, w = got[n][rows], want[n][rows]
        assert g.shape == w.shape and g.dtype == w.dtype, (where, n, g.shape, w.shape, g.dtype, w.dtype)
        if n == "reward":
            g, w = g.view(np.uint64), w.view(np.uint64)
        bad = np.argwhere(g != w)
        assert not len(bad), (where, n, "board", int(np.asarray(rows)[bad[0][0]]), "replica", int(bad[0][1]),
                              g[tuple(bad[0])], w[tuple(bad[0])], len(bad))


def guards(want, rows, reps):
    """What a parity case contains, from the twins: (some replica done, some not done, some board
    whose replicas differ in first action or return)."""
    d = want["done"][rows]
    differ = False
    if reps > 1:
        for n in ("reward", "first_def", "first_atk"):
            if n in want:
                v = want[n][rows].reshape(len(rows), reps, -1)
                differ = differ or bool((v != v[:, :1]).any())
    return bool((d != 0).any()), bool((d == 0).any()), differ


def poison_probe(eng, reps):
    """The engine's probe buffers at ``reps``, every byte POISON; returns the (B, reps) views."""
    _, out, _ = eng._probe_prepare(1, reps, 0, 0.0, 0.0, True)
    for t in out.values():
        if t is not None:
            t.view(torch.uint8).fill_(POISON)
    return out


def rows_poisoned(out, rows):
    """Every byte of the rows ``rows`` (board ids) of the probe's tensors is still POISON."""
    for n, t in out.items():
        if t is not None and len(rows):
            b = t.view(torch.uint8).cpu().numpy().reshape(t.shape[0], -1)[rows]
            assert (b == POISON).all(), (n, np.asarray(rows)[np.flatnonzero((b != POISON).any(axis=1))[:4]])


def everything(eng, extra=None):
    """Every byte a probe must leave alone, by name: streamutil's snapshot (every step output
    tensor with the observation, the exported state with the opponent stream's raw words, position
    and lazy-twist boundary, both streams as td_get_*_state gives them, flags, episode records and
    statistics) and the playout's output tensors."""
    s = SU.snapshot(eng, extra)
    for k, v in eng.export_state().items():  # the export's own bytes too (the snapshot zeroes dead slots)
        s["raw." + k] = np.ascontiguousarray(v).view(np.uint8).reshape(eng.B, -1)
    for n, t in (getattr(eng, "_playout_buf", None) or {}).items():
        if t is not None:
            s["playout." + n] = np.ascontiguousarray(t.view(torch.uint8).cpu().numpy()).reshape(eng.B, -1)
    return s


def unchanged(before, after, where):
    assert set(before) == set(after), (where, sorted(set(before) ^ set(after)))
    for k in sorted(before):
        if k == SU.SUM:
            assert before[k] == after[k], (where, k)
        else:
            assert np.array_equal(before[k], after[k]), (where, k, np.flatnonzero((before[k] != after[k]).any(axis=1))[:4])
