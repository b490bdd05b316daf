"""Legal-action sampling restated in numpy: the reference of ``TDEngine.sample_actions`` and of
``TDEngine.sample_weighted``.

The rules of csrc/td_sample.h -- splitmix64 over (seed, ticket, board id, draw); uniform: an idle
draw and a multiply-shift pick per side; weighted: float32 weights quantised to integers, an
integer total and a 64-bit multiply-shift threshold against the prefix sums -- applied to the
masks of ``gym_TD.masks.reference_masks``.
"""
import numpy as np

M64 = (1 << 64) - 1
DEF_IDLE, DEF_PICK, ATK_IDLE, ATK_PICK = range(4)  # the draw j


def sm(z):
    """splitmix64's output step on z + 0x9E3779B97F4A7C15 (mod 2^64)."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def word(seed, ticket, b, j):
    """The 64-bit word of draw j of board b under (seed, ticket)."""
    return sm((sm((sm(int(seed) & M64) + int(ticket)) & M64) + 4 * int(b) + int(j)) & M64)


def u32(seed, ticket, b, j):
    return word(seed, ticket, b, j) >> 32


def idle_units(p):
    """An idle probability as the call takes it: an int is units of 2^-32, a float a probability."""
    if isinstance(p, (int, np.integer)) and not isinstance(p, (bool, np.bool_)):
        if not 0 <= int(p) <= 0xFFFFFFFF:
            raise ValueError("idle probability in units of 2^-32 must be in [0, 2^32), not %r" % (p,))
        return int(p)
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("idle probability must be in [0, 1], not %r" % (p,))
    return min(2 ** 32 - 1, int(p * 2 ** 32))


def _choose(cand, seed, ticket, b, j_idle, j_pick, idle):
    """The chosen candidate, or None: nothing is legal, or the idle draw fires."""
    n = len(cand)
    if n == 0 or u32(seed, ticket, b, j_idle) < idle:
        return None
    return int(cand[(u32(seed, ticket, b, j_pick) * n) >> 32])


def reference_playout(env, state_of, L, cfg, hp, mode, seed, ticket, b, steps, def_idle=0, atk_idle=0, cap=True):
    """The CPU statement of ``TDEngine.playout`` for one board: ``env`` (an oracle env of the
    step's interface: ``step(def_act=..., atk_act=...)`` -> (obs, reward, done, info)) is played
    on for up to ``steps`` sub-steps; sub-step j steps it with ``reference_sample`` over
    ``reference_masks(state_of(env))`` at ticket + j (mod 2^64) under board id ``b``, and the
    playout stops after the sub-step that ends the episode (the env is left there: a caller that
    mirrors auto-reset resets it).  Discrete actions only.

    state_of: env -> the canonical state dict ``reference_masks`` reads (with ``num_roads``).
    Returns a dict: ``reward`` (r_0, then added left to right in f64), ``done``, ``steps_run``,
    ``first_def`` / ``first_atk`` (sub-step 0's actions; None for a side the mode lacks),
    ``info`` (the last sub-step's) and ``events``: per sub-step a dict with ``def`` (the action
    index or None), ``def_n``, ``atk`` ((road, type) or None), ``atk_n`` (the candidate counts;
    None for a side the mode lacks).
    """
    from .masks import reference_masks
    A = 6 * L * L
    total, done, info, run = 0.0, False, None, 0
    first_def = first_atk = None
    events = []
    for j in range(int(steps)):
        dm, _, am = reference_masks(state_of(env), L, cfg, hp, mode, False, cap=cap)
        d, a, dn, an = reference_sample(dm, am, seed, (int(ticket) + j) & M64, b, def_idle, atk_idle, L, False)
        if j == 0:
            first_def, first_atk = d, a
        kw = {}
        if mode != "atk":
            kw["def_act"] = d
        if mode != "def":
            kw["atk_act"] = a
        _, r, done, info = env.step(**kw)
        rt = None
        if a is not None:
            roads = np.flatnonzero(a[:, 0] != 4)
            rt = (int(roads[0]), int(a[roads[0], 0])) if len(roads) else None
        events.append({"def": None if d is None or d == A else int(d), "def_n": dn, "atk": rt, "atk_n": an})
        total = float(r) if j == 0 else total + float(r)
        run = j + 1
        if done:
            break
    return {"reward": total, "done": bool(done), "steps_run": run, "first_def": first_def, "first_atk": first_atk,
            "info": info, "events": events}


def reference_probe(env, steps, reps, state_of, L, cfg, hp, mode, seed, ticket, b, def_idle=0, atk_idle=0, cap=True):
    """The CPU statement of ``TDEngine.probe`` for one board: replica r (0 <= r < ``reps``) is
    ``reference_playout`` at ticket + r * steps (mod 2^64) on a deep copy of ``env`` -- its state
    and its opponent's stream as they are now, so every replica starts from the same stream
    position --, and ``env`` itself is never stepped.  The other arguments are
    ``reference_playout``'s.  Returns the list of the replicas' dicts."""
    import copy
    steps = int(steps)
    return [reference_playout(copy.deepcopy(env), state_of, L, cfg, hp, mode, seed, (int(ticket) + r * steps) & M64, b,
                              steps, def_idle, atk_idle, cap)
            for r in range(int(reps))]


def reference_sample(def_mask, atk_mask, seed, ticket, b, def_idle, atk_idle, L, multi):
    """(def_act, atk_act, def_count, atk_count) of board b, in the step's formats.

    def_mask: reference_masks' row, (6 L^2 + 1,) or (6, L, L) with ``multi``, or None (TD-atk);
    atk_mask: (3, 5) or None (TD-def).  def_idle / atk_idle: units of 2^-32 (ints) or
    probabilities (floats).  def_act: int (6 L^2 = the no-op) or int64 (6, L, L) with one flag
    at most; atk_act: int64 (3, 8), all 4 but the chosen road's first slot.  A side without a
    mask gives None for its action and its count.
    """
    A = 6 * L * L
    d_act = a_act = d_n = a_n = None
    if def_mask is not None:
        cand = np.flatnonzero(np.asarray(def_mask).reshape(-1)[:A])
        d_n = len(cand)
        k = _choose(cand, seed, ticket, b, DEF_IDLE, DEF_PICK, idle_units(def_idle))
        if multi:
            d_act = np.zeros((6, L, L), dtype=np.int64)
            if k is not None:
                d_act.reshape(-1)[k] = 1
        else:
            d_act = A if k is None else k
    if atk_mask is not None:
        cand = np.flatnonzero(np.asarray(atk_mask)[:, :4].reshape(-1))  # road * 4 + t
        a_n = len(cand)
        k = _choose(cand, seed, ticket, b, ATK_IDLE, ATK_PICK, idle_units(atk_idle))
        a_act = np.full((3, 8), 4, dtype=np.int64)
        if k is not None:
            a_act[k // 4, 0] = k % 4
    return d_act, a_act, d_n, a_n


def quantize(w):
    """q of td_sample_weighted, elementwise: 0 unless w > 0 (NaN, -0, negatives, 0), else
    trunc(min(w, 1) * 2^31) with the product taken in float32 (exact: a power of two).  +inf and
    everything above 1 give 2^31; subnormals and everything below 2^-31 give 0.  ``w`` is taken as
    float32; returns int64 of the same shape."""
    w = np.asarray(w, dtype=np.float32)
    pos = w > 0  # (False for NaN)
    c = np.where(pos, np.minimum(np.where(pos, w, np.float32(0)), np.float32(1)), np.float32(0)).astype(np.float32)
    return (c * np.float32(2.0 ** 31)).astype(np.float32).astype(np.int64)


def weights_from_logits(logits):
    """exp(l - row max) in float32 over the last axis: weights in (0, 1] whose row maximum is
    exactly 1, as ``sample_weighted`` takes them.  A torch tensor gives a torch tensor (on its
    device), anything else a numpy array."""
    try:
        import torch
    except ImportError:  # (the reference alone needs numpy only)
        torch = None
    if torch is not None and isinstance(logits, torch.Tensor):
        x = logits.to(torch.float32)
        return torch.exp(x - x.max(dim=-1, keepdim=True).values)
    x = np.asarray(logits, dtype=np.float32)
    return np.exp(x - x.max(axis=-1, keepdims=True)).astype(np.float32)


def pick_weighted(m, w64):
    """The rule over the masses ``m`` (ints, 0 where illegal, the always-legal entry last) and the
    draw's 64-bit word: (pick, (m(pick), S)), or (the last entry, (0, 0)) when S == 0."""
    m = [int(x) for x in m]
    S = sum(m)
    if S == 0:
        return len(m) - 1, (0, 0)
    r = (int(w64) * S) >> 64
    c = 0
    for e, x in enumerate(m):
        c += x
        if c > r:
            return e, (x, S)
    raise AssertionError("r < S")


def reference_sample_weighted(def_mask, atk_mask, def_w, atk_w, seed, ticket, b, L):
    """(def_act, atk_act, def_mass, atk_mass) of board b under td_sample_weighted's rule.

    def_mask: reference_masks' discrete row (6 L^2 + 1,), or None (TD-atk); atk_mask: (3, 5) or
    None (TD-def).  def_w: the board's (6 L^2 + 1,) float32 weights, the no-op last; atk_w: its
    (13,) weights, entry road * 4 + t and "nothing" last.  def_act: int (6 L^2 = the no-op);
    atk_act: int64 (3, 8), all 4 but the chosen road's first slot; the masses: (m(chosen), S) as
    ints, (0, 0) when S == 0.  A side without a mask gives None for its action and its mass.
    """
    A = 6 * L * L
    d_act = a_act = d_mass = a_mass = None
    if def_mask is not None:
        legal = np.asarray(def_mask).reshape(-1)[:A + 1] != 0
        legal[A] = True  # the no-op
        m = np.where(legal, quantize(np.asarray(def_w, dtype=np.float32).reshape(-1)[:A + 1]), 0)
        d_act, d_mass = pick_weighted(m, word(seed, ticket, b, DEF_PICK))
    if atk_mask is not None:
        legal = np.append(np.asarray(atk_mask)[:, :4].reshape(-1) != 0, True)  # road * 4 + t, then "nothing"
        m = np.where(legal, quantize(np.asarray(atk_w, dtype=np.float32).reshape(-1)[:13]), 0)
        e, a_mass = pick_weighted(m, word(seed, ticket, b, ATK_PICK))
        a_act = np.full((3, 8), 4, dtype=np.int64)
        if e < 12:
            a_act[e // 4, 0] = e % 4
    return d_act, a_act, d_mass, a_mass
