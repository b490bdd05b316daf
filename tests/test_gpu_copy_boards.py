"""td_copy_boards / TDEngine.copy_boards / TDVecEnv.fork on the device.

The step kernels are pinned to the oracle elsewhere (test_gpu_envs.py, test_gpu_crowded.py,
test_gpu_frame_skip.py ...), so the yardstick here is "the clone equals its source": the
exported state with the slots past the counts zeroed, the header and the opponent's 626 stream
words word for word, the observation row byte for byte, and -- stepped on with the same actions
-- every output tensor of every later step, bit for bit.  (The hot record's pre-drawn outputs
are in no export: they are compared through those later steps, whose draws they are.)  Boards that no call names must not move at
all.  No oracle runs here; every case is a few hundred steps of at most 32 small boards.
"""
import copy

import numpy as np
import pytest
import torch

import skiputil as S
import test_kernel_meta as KM

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU too, so skip cleanly
    pytest.skip("needs a GPU", allow_module_level=True)

from gym_TD import _lib  # noqa: E402
from gym_TD import envs as E  # noqa: E402
from gym_TD import params as P  # noqa: E402
from gym_TD.engine import TDEngine  # noqa: E402

lib = _lib.lib
OUTPUTS = ("obs", "reward", "done", "win", "allow_next", "cooldowns", "ep_return", "ep_len", "real_def", "fail_def",
           "real_atk", "fail_atk")
FLAG_NO_LAYOUT = 8


# ------------------------------------------------------------------ helpers
def _cfg(**over):
    cfg = copy.deepcopy(P.config)
    for k, v in over.items():
        setattr(cfg, k, copy.deepcopy(v))
    return cfg


def _engine(L, B, mode="def", multi=False, seed0=900, cfg=None, autoreset=False, **kw):
    seeds = list(range(seed0, seed0 + B))
    eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=autoreset, cfg=cfg, **kw)
    eng.reset_all()
    return eng


def _draw(rng, eng):
    """Uniform random actions for every board (multi-action: sparse flags)."""
    L, B = eng.L, eng.B
    d = a = None
    if eng.mode != "atk":
        d = ((rng.random_sample((B, 6, L, L)) < 0.02).astype(np.int64) if eng.multi
             else rng.randint(0, 6 * L * L + 1, size=B).astype(np.int64))
    if eng.mode != "def":
        a = rng.randint(0, 5, size=(B, 3, 8)).astype(np.int64)
    return d, a


def _mirror(acts, src, dst):
    """The clones take their sources' actions."""
    for x in acts:
        if x is not None:
            x[dst] = x[src]
    return acts


def _step(eng, acts):
    d, a = acts
    eng.step(def_act=None if d is None else torch.from_numpy(d), atk_act=None if a is None else torch.from_numpy(a))


def _rows(t, idx):
    """Rows idx of a device tensor as bytes."""
    return t[torch.as_tensor(idx, device=t.device, dtype=torch.long)].contiguous().view(torch.uint8)


def _differing_outputs(eng, src, dst, names=OUTPUTS):
    """The output tensors whose rows dst are not bit for bit the rows src."""
    bad = []
    for n in names:
        t = getattr(eng, n)
        if t is not None and not torch.equal(_rows(t, dst), _rows(t, src)):
            bad.append(n)
    return bad


def _live(st):
    """The exported arrays with the slots beyond n_en / n_tw zeroed (as test_gpu_frame_skip.py)."""
    st = {k: v.copy() for k, v in st.items()}
    for names, n, cap in ((("en_lp", "en_mg", "en_inf"), st["hdr"]["n_en"], _lib.ECAP),
                          (("tw_cd", "tw_inf"), st["hdr"]["n_tw"], _lib.TCAP)):
        dead = np.arange(cap)[None, :] >= n[:, None]
        for name in names:
            st[name][dead] = 0
    return st


def _assert_clones(eng, src, dst, tag):
    """State, header, opponent stream, flags and observation row of every dst equal its src's."""
    st = _live(eng.export_state())
    for name, a in st.items():
        for s, d in zip(src, dst):
            assert a[d].tobytes() == a[s].tobytes(), (tag, name, s, d)
    fl = eng.flags()
    assert (fl[dst] == fl[src]).all(), (tag, fl.tolist())
    assert torch.equal(_rows(eng.obs, dst), _rows(eng.obs, src)), (tag, "obs")
    return st


def _snapshot(eng):
    return eng.export_state(), eng.flags(), eng.obs.cpu().numpy().copy()


def _assert_untouched(eng, before, boards, tag):
    """Boards `boards`: raw state (dead slots included), flags and observation bytes as in `before`."""
    st0, fl0, ob0 = before
    st, fl, ob = _snapshot(eng)
    boards = np.asarray(boards, dtype=np.int64)
    for name in st0:
        assert st[name][boards].tobytes() == st0[name][boards].tobytes(), (tag, name)
    assert (fl[boards] == fl0[boards]).all(), tag
    assert ob[boards].tobytes() == ob0[boards].tobytes(), (tag, "obs")


def _fan(B):
    """The pairs of the grid: boards 0 .. B/4-1 to B/2 .. 3B/4-1 and, in the same call, board 0
    to the B/8 boards after them (B = 32: 0..7 -> 16..23 and 0 -> 24..27)."""
    q = B // 4
    src = list(range(q)) + [0] * (B // 8)
    dst = list(range(B // 2, B // 2 + q)) + list(range(3 * B // 4, 3 * B // 4 + B // 8))
    return src, dst


# ------------------------------------------------------------------ 1 clone equals source, nothing else moves
GRID = [(10, 32, m, False, k) for m in ("def", "atk", "2p") for k in ("large", "small", "small2")] + \
       [(20, 8, "2p", True, "auto"), (12, 8, "def", False, "auto"), (30, 8, "def", False, "auto")]


@pytest.mark.parametrize("L,B,mode,multi,kernel", GRID)
def test_clone_equals_source_and_nothing_else_moves(L, B, mode, multi, kernel):
    eng = _engine(L, B, mode, multi, step_kernel=kernel)
    try:
        rng = np.random.RandomState(11)
        for _ in range(150):
            _step(eng, _draw(rng, eng))
        src, dst = _fan(B)
        others = [b for b in range(B) if b not in dst]
        assert dst[0] - 1 in others and (dst[-1] + 1 in others or dst[-1] == B - 1)  # the rows' line neighbours
        before = _snapshot(eng)
        np_dst = eng.get_np_state(dst[0])
        assert eng.copy_boards(src, dst) is eng.obs
        _assert_clones(eng, src, dst, (L, mode, kernel, "copy"))
        _assert_untouched(eng, before, others, (L, mode, kernel))
        assert np.array_equal(eng.get_np_state(dst[0]), np_dst)  # random_agent=True: its own layout stream
        masks = eng.action_mask(code=True)
        for name, m in masks.items():
            assert torch.equal(_rows(m, dst), _rows(m, src)), (L, mode, kernel, "mask", name)
        for k in range(120):
            _step(eng, _mirror(_draw(rng, eng), src, dst))
            bad = _differing_outputs(eng, src, dst)
            assert not bad, (L, mode, kernel, k, bad)
        _assert_clones(eng, src, dst, (L, mode, kernel, "end"))
    finally:
        eng.close()


# ------------------------------------------------------------------ 2 full and crowded lists
def test_full_and_crowded_lists():
    """TD-2p, 8 boards of 10x10 under a config that lets the lists fill by the reference's own
    rules (money for exactly 128 enemies of cost 1 that barely move; towers that block only
    their 4-neighbourhood): board 0 ends with exactly 128 enemies, board 1 with 72 (the slots
    past 16 and past 64), board 2 with 32 towers; board 3 is reset right before the copy (a
    fresh board: step 0, no enemy, no tower).  Copied to 4 .. 7.

    The config is crowdutil's FULL and TOWERS put together.  crowdutil's scenarios themselves
    draw their actions from the Python oracle's envs, stepped beside the device (seconds per
    scenario), and which board holds how many enemies when is the oracle's to say; here the
    schedule is fixed, so the counts below are exact and asserted, and the yardstick is the
    clone's source, which tests/test_gpu_crowded.py holds to the oracle on those scenarios."""
    L, B = 10, 8
    cfg = _cfg(attacker_init_cost=128, attacker_cost_init_rate=0, attacker_cost_final_rate=0,
               enemy_cost=[[1, 1]] * 4, enemy_speed=[[.03, .03]] * 4, tower_distance=1, defender_init_cost=300,
               max_cost=400, defender_cost_rate=8, base_LP=10 ** 6)
    eng = _engine(L, B, "2p", False, seed0=4000, cfg=cfg)
    try:
        rng = np.random.RandomState(3)
        empty_d = 6 * L * L
        for k in range(120):
            st = eng.export_state()
            if k >= 20 and st["hdr"]["n_tw"][2] == _lib.TCAP:
                break
            d = np.full(B, empty_d, dtype=np.int64)
            a = np.full((B, 3, 8), 4, dtype=np.int64)
            a[0, 0] = rng.randint(0, 4, size=8)  # eight summons a step on road 0 until the money is gone
            if k < 9:
                a[1, 0] = rng.randint(0, 4, size=8)
            free = np.flatnonzero((st["cells"][2] >> 24) == 0)
            if st["hdr"]["n_tw"][2] < _lib.TCAP and len(free):
                d[2] = (k % 4) * L * L + int(free[0])
            _step(eng, (d, a))
        mask = np.zeros(B, dtype=np.uint8)
        mask[3] = 1
        assert eng.reset(mask)[1] == []
        hdr = eng.export_state()["hdr"]
        assert hdr["steps"][3] == 0 and hdr["steps"][2] > 30
        assert hdr["n_en"][:4].tolist() == [128, 72, 0, 0] and hdr["n_tw"][:4].tolist() == [0, 0, 32, 0], \
            (hdr["n_en"].tolist(), hdr["n_tw"].tolist())
        src, dst = [0, 1, 2, 3], [4, 5, 6, 7]
        eng.copy_boards(src, dst)
        st = _assert_clones(eng, src, dst, "crowded copy")
        assert st["hdr"]["n_en"][4:].tolist() == [128, 72, 0, 0] and st["hdr"]["n_tw"][4:].tolist() == [0, 0, 32, 0]
        assert st["en_lp"][4][127] > 0 and st["en_lp"][5][71] > 0 and st["en_lp"][5][72] == 0  # live slots came along
        for k in range(20):
            _step(eng, _mirror(_draw(rng, eng), src, dst))
            bad = _differing_outputs(eng, src, dst)
            assert not bad, (k, bad)
        _assert_clones(eng, src, dst, "crowded end")
    finally:
        eng.close()


# ------------------------------------------------------------------ 3 formats and retention
def test_float16_rows():
    eng = _engine(10, 32, "def", obs_dtype=torch.float16)
    try:
        rng = np.random.RandomState(5)
        for _ in range(60):
            _step(eng, _draw(rng, eng))
        src, dst = _fan(32)
        before = _snapshot(eng)
        eng.copy_boards(src, dst)
        assert eng.obs.dtype == torch.float16
        _assert_clones(eng, src, dst, "f16")
        _assert_untouched(eng, before, [b for b in range(32) if b not in dst], "f16")
        for k in range(10):
            _step(eng, _mirror(_draw(rng, eng), src, dst))
            assert not _differing_outputs(eng, src, dst), k
    finally:
        eng.close()


@pytest.mark.parametrize("how", ["into_obs", "no_obs", "second_buffer"])
def test_retention_follows_the_copy(how):
    """A retaining engine and its non-retaining twin (which writes every byte, every step) do
    the same steps, the same copy and 10 more steps: the observation buffers are equal byte
    for byte after the copy and after every step.  no_obs: the copy writes nothing, so the
    retaining engine's next step must write every byte; second_buffer: the copy writes into
    a buffer that is not the retained one, which must leave the retained one behind as well."""
    engs = [_engine(10, 32, "def", retain_obs=r) for r in (True, False)]
    try:
        if not engs[0].retain_obs:
            pytest.skip("TD_RETAIN_OBS=0: no engine retains")
        assert lib.td_retained_obs(engs[0]._h) == engs[0].obs.data_ptr() and not lib.td_retained_obs(engs[1]._h)
        rng = np.random.RandomState(8)
        src, dst = _fan(32)
        s32, d32 = np.asarray(src, dtype=np.int32), np.asarray(dst, dtype=np.int32)
        other = [torch.zeros_like(e.obs) for e in engs]
        for k in range(51):
            acts = _draw(rng, engs[0]) if k < 40 else _mirror(_draw(rng, engs[0]), src, dst)
            if k == 40:
                for e, buf in zip(engs, other):
                    if how == "into_obs":
                        e.copy_boards(src, dst)
                    elif how == "no_obs":
                        e.copy_boards(src, dst, write_obs=False)
                    else:
                        _lib.check(lib.td_copy_boards(e._h, s32.ctypes.data, d32.ctypes.data, len(src), buf.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream))
                if how == "second_buffer":
                    assert torch.equal(_rows(other[0], dst), _rows(engs[0].obs, src))
                    assert torch.equal(other[0].view(torch.uint8), other[1].view(torch.uint8))
                    assert not bool(other[0][[b for b in range(32) if b not in dst]].view(torch.uint8).any())
                assert lib.td_retained_obs(engs[0]._h) == engs[0].obs.data_ptr()
                assert torch.equal(engs[0].obs.view(torch.uint8), engs[1].obs.view(torch.uint8)), (how, "copy")
                if how == "into_obs":
                    assert torch.equal(_rows(engs[0].obs, dst), _rows(engs[0].obs, src))
            for e in engs:
                _step(e, acts)
            assert torch.equal(engs[0].obs.view(torch.uint8), engs[1].obs.view(torch.uint8)), (how, k)
            if k >= 40:
                assert not _differing_outputs(engs[0], src, dst), (how, k)
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------------ 4 frame skip
def test_frame_skip_clone():
    eng = _engine(10, 32, "def", frame_skip=4)
    try:
        rng = np.random.RandomState(9)
        for _ in range(10):
            _step(eng, _draw(rng, eng))
        src, dst = _fan(32)
        eng.copy_boards(src, dst)
        _assert_clones(eng, src, dst, "skip")
        for k in range(10):
            _step(eng, _mirror(_draw(rng, eng), src, dst))
            assert not _differing_outputs(eng, src, dst), k
        _assert_clones(eng, src, dst, "skip end")
    finally:
        eng.close()


# ------------------------------------------------------------------ 5 auto-reset, both stream modes
def _layout_of(eng, st, b):
    m, start, end = eng.map_planes(b, st)
    return int(st["hdr"]["num_roads"][b]), m[:6].tobytes(), tuple(map(tuple, start)), tuple(end)


def test_autoreset_random_agent_true_keeps_the_destinations_layout_sequence():
    """One-LP bases (episodes end within a few dozen steps) and a twin engine on the same seeds
    that never copies.  A clone is its source up to and including the step that ends the
    episode (whose observation is already each board's own next layout); from then on board
    dst runs the layouts board dst of the twin runs, in the same order: the copy touched
    neither the staged layouts nor the layout stream."""
    L, B = 10, 16
    a, t = (_engine(L, B, "def", cfg=_cfg(**S.RECIPE), autoreset=True) for _ in range(2))
    try:
        rng = np.random.RandomState(21)
        src, dst = [0, 1, 2, 3], [8, 9, 10, 11]
        for _ in range(10):
            acts = _draw(rng, a)
            _step(a, acts)
            _step(t, acts)
        assert torch.equal(a.obs.view(torch.uint8), t.obs.view(torch.uint8))
        a.copy_boards(src, dst)
        _assert_clones(a, src, dst, "autoreset copy")
        live = dict(zip(src, dst))  # pairs whose episode still runs
        seq_a = {d: [] for d in dst}
        seq_t = {d: [] for d in dst}
        for k in range(600):
            acts = _draw(rng, a)
            _step(t, acts)
            _step(a, _mirror(acts, list(live.keys()), list(live.values())) if live else acts)
            done_a, done_t = a.done.cpu().numpy(), t.done.cpu().numpy()
            if live:
                s_, d_ = list(live.keys()), list(live.values())
                running = [i for i, s in enumerate(s_) if not done_a[s]]
                bad = _differing_outputs(a, s_, d_, [n for n in OUTPUTS if n != "obs"])
                assert not bad, (k, bad)  # the finishing step included
                if running:
                    rs, rd = [s_[i] for i in running], [d_[i] for i in running]
                    assert torch.equal(_rows(a.obs, rd), _rows(a.obs, rs)), k
            sa = st = None
            for d in dst:
                if done_a[d]:
                    sa = sa or a.export_state()
                    seq_a[d].append(_layout_of(a, sa, d))
                if done_t[d]:
                    st = st or t.export_state()
                    seq_t[d].append(_layout_of(t, st, d))
            for s in [s for s in live if done_a[s]]:
                del live[s]
            if not live and all(len(seq_a[d]) >= 2 and len(seq_t[d]) >= 2 for d in dst):
                break
        assert not live
        for d in dst:
            n = min(len(seq_a[d]), len(seq_t[d]))
            assert n >= 2 and seq_a[d][:n] == seq_t[d][:n], (d, n)
        assert (a.flags() == 0).all() and (t.flags() == 0).all()
    finally:
        a.close()
        t.close()


def test_autoreset_random_agent_false_clone_follows_through_resets():
    """random_agent=False: the numpy stream is the opponent's too and is copied, so the clone
    stays its source through the auto-resets (same draws, same layouts)."""
    L, B = 10, 16
    eng = _engine(L, B, "def", cfg=_cfg(**S.RECIPE), autoreset=True, random_agent=False)
    try:
        rng = np.random.RandomState(22)
        for _ in range(10):
            _step(eng, _draw(rng, eng))
        src, dst = [0, 1, 2, 3, 0], [8, 9, 10, 11, 12]
        np_before = eng.get_np_state(5)
        eng.copy_boards(src, dst)
        _assert_clones(eng, src, dst, "np copy")
        for s, d in zip(src, dst):
            assert np.array_equal(eng.get_np_state(d), eng.get_np_state(s)), (s, d)
        assert np.array_equal(eng.get_np_state(5), np_before)
        ends = np.zeros(B, dtype=int)
        for k in range(400):
            _step(eng, _mirror(_draw(rng, eng), src, dst))
            bad = _differing_outputs(eng, src, dst)
            assert not bad, (k, bad)
            ends += eng.done.cpu().numpy()
            if (ends[src] >= 3).all():
                break
        assert (ends[src] >= 3).all(), ends.tolist()
        _assert_clones(eng, src, dst, "np end")
    finally:
        eng.close()


# ------------------------------------------------------------------ 6 config epochs
def test_config_epochs_are_kept():
    """Entities created under an earlier paramConfig keep its values in the clone as in the
    source (their epoch tags travel as they are); the host path retags to the current epoch,
    so an imported copy of the same boards does NOT stay equal -- pinned once, as the header
    states it.  Then 300 more epochs: td_set_config recycles blocks, counting the clones."""
    L, B = 10, 16
    mk = lambda i: S.cfg_at(i, copy.deepcopy(P.config))  # noqa: E731
    a = _engine(L, B, "def", cfg=mk(0), seed0=6200)
    c = _engine(L, B, "def", cfg=mk(0), seed0=6200)
    try:
        rng = np.random.RandomState(31)
        from oracle import policies
        def draw():  # builds on free cells mostly, so towers of several epochs stand
            st = a.export_state()
            road = [((st["cells"][b] & 1) != 0).reshape(L, L) for b in range(B)]
            return np.array([policies.discrete_def(rng, L, road[b], 0.7) for b in range(B)], dtype=np.int64), None
        for _ in range(20):
            _step(a, draw())
        a.set_config(mk(1))
        c.set_config(mk(1))
        for _ in range(30):
            _step(a, draw())
        src, dst = list(range(8)), list(range(8, 16))
        st = a.export_state()
        tags = np.concatenate([(st["en_inf"][b][:st["hdr"]["n_en"][b]] >> 24) for b in src] +
                              [(st["tw_inf"][b][:st["hdr"]["n_tw"][b]] >> 24) for b in src])
        assert len(set(tags.tolist())) >= 2, tags.tolist()  # entities of both epochs are alive
        a.copy_boards(src, dst)
        _assert_clones(a, src, dst, "epochs copy")
        c.import_state(a.export_state())  # (the opponent streams come with it)
        a.set_config(mk(2))
        c.set_config(mk(2))
        differs = False
        for k in range(60):
            acts = _mirror(draw(), src, dst)
            _step(a, acts)
            _step(c, acts)
            bad = _differing_outputs(a, src, dst)
            assert not bad, (k, bad)
            differs = differs or not torch.equal(a.obs.view(torch.uint8), c.obs.view(torch.uint8))
        assert differs  # the imported boards read the current epoch's values
        _assert_clones(a, src, dst, "epochs 60")
        for i in range(3, 303):
            a.set_config(mk(i))  # (raises TDError if no block can be recycled)
            _step(a, _mirror(_draw(rng, a), src, dst))
            if i % 25 == 0:
                assert not _differing_outputs(a, src, dst), i
        assert not _differing_outputs(a, src, dst)
    finally:
        a.close()
        c.close()


# ------------------------------------------------------------------ 7 refusals
def _raw_copy(eng, src, dst, n, obs=True):
    s = None if src is None else np.ascontiguousarray(src, dtype=np.int32)
    d = None if dst is None else np.ascontiguousarray(dst, dtype=np.int32)
    return lib.td_copy_boards(eng._h, None if s is None else s.ctypes.data, None if d is None else d.ctypes.data, n,
                              eng.obs.data_ptr() if obs else None, torch.cuda.current_stream().cuda_stream)


def test_refusals_change_nothing():
    B = 16
    engs = [_engine(10, B, "def", retain_obs=r) for r in (True, False)]
    try:
        rng = np.random.RandomState(41)
        for _ in range(10):
            acts = _draw(rng, engs[0])
            for e in engs:
                _step(e, acts)
        e = engs[0]
        before = _snapshot(e)
        kept = lib.td_retained_obs(e._h)
        bad = [("NULL src", None, [1], 1), ("NULL dst", [0], None, 1), ("n < 0", [0], [1], -1),
               ("n > B", [0] * (B + 1), list(range(1, B)) + [1, 2], B + 1), ("src < 0", [-1], [1], 1),
               ("src = B", [B], [1], 1), ("dst < 0", [0], [-1], 1), ("dst = B", [0, 1], [2, B], 2),
               ("dst twice", [0, 1], [5, 5], 2), ("self", [3], [3], 1), ("src and dst", [0, 1], [1, 2], 2)]
        for what, s, d, n in bad:
            for obs in (True, False):
                assert _raw_copy(e, s, d, n, obs) < 0, what
                assert lib.td_last_error().startswith(b"td_copy_boards"), (what, lib.td_last_error())
        with pytest.raises(_lib.TDError):
            e.copy_boards([0, 1], [2, 2])
        with pytest.raises(ValueError):
            e.copy_boards([0, 1], [2])
        assert _raw_copy(e, [0], [1], 0) == 0 and _raw_copy(e, None, None, 0) == 0  # n == 0: nothing to do
        assert lib.td_copy_boards(None, None, None, 0, None, None) < 0
        _assert_untouched(e, before, list(range(B)), "refusals")
        assert lib.td_retained_obs(e._h) == kept
        for k in range(5):  # the retained buffer is still what the engine thinks it is
            acts = _draw(rng, e)
            for x in engs:
                _step(x, acts)
            assert torch.equal(engs[0].obs.view(torch.uint8), engs[1].obs.view(torch.uint8)), k
        # a repeated source is the point of the call
        e.copy_boards(torch.tensor([0, 0, 0], device=e.device), np.array([5, 6, 7]))
        _assert_clones(e, [0, 0, 0], [5, 6, 7], "fan-out")
    finally:
        for x in engs:
            x.close()


def test_source_without_an_episode():
    """A board whose reset failed (a failing seed of the golden road table) is copied like any
    other: the destination's observation row keeps its previous bytes, and on the next step the
    destination reports what the source reports."""
    import goldens as G
    rows = G.load_roadgen()["10"]
    err = sorted(int(s) for s in rows if "err" in rows[s])[0]
    good = sorted(int(s) for s in rows if "err" not in rows[s])[:7]
    seeds = [err] + good
    eng = TDEngine(10, 8, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=False)
    try:
        _, failed = eng.reset()
        assert failed == [0]
        rng = np.random.RandomState(2)
        for _ in range(5):
            _step(eng, _draw(rng, eng))
        before = _snapshot(eng)
        eng.copy_boards([0, 1], [5, 6])
        st = _live(eng.export_state())
        for name, a in st.items():
            assert a[5].tobytes() == a[0].tobytes() and a[6].tobytes() == a[1].tobytes(), name
        ob = eng.obs.cpu().numpy()
        assert ob[5].tobytes() == before[2][5].tobytes() and ob[5].any()  # left unwritten
        assert ob[6].tobytes() == ob[1].tobytes()
        _assert_untouched(eng, before, [0, 1, 2, 3, 4, 7], "no episode")
        _step(eng, _mirror(_draw(rng, eng), [0, 1], [5, 6]))
        assert not _differing_outputs(eng, [0, 1], [5, 6])
        assert bool(eng.done[5]) and not bool(eng.obs[5].view(torch.uint8).any())
        fl = eng.flags()
        assert fl[5] == fl[0] == FLAG_NO_LAYOUT
    finally:
        eng.close()


# ------------------------------------------------------------------ 8 no host synchronisation needed
def test_back_to_back_equals_synchronised():
    """step, copy, step, copy ... issued back to back on one stream (more copies than the
    handle has index slots, each with other pairs, the caller's arrays overwritten right after
    each call) against the same sequence with a device synchronise after every call."""
    L, B = 10, 32
    pairs = [([i % 8, (i + 3) % 8], [8 + 2 * i, 9 + 2 * i]) for i in range(7)]
    rng = np.random.RandomState(51)
    engs = [_engine(L, B, "2p") for _ in range(2)]
    try:
        acts = [_draw(rng, engs[0]) for _ in range(len(pairs) + 1)]
        dev = [tuple(None if x is None else torch.from_numpy(x).to(engs[0].device) for x in a) for a in acts]
        for sync, e in zip((False, True), engs):
            torch.cuda.synchronize()
            s = np.zeros(2, dtype=np.int32)
            d = np.zeros(2, dtype=np.int32)
            for i, (ps, pd) in enumerate(pairs):
                e.step(def_act=dev[i][0], atk_act=dev[i][1])
                if sync:
                    torch.cuda.synchronize()
                s[:], d[:] = ps, pd
                _lib.check(lib.td_copy_boards(e._h, s.ctypes.data, d.ctypes.data, 2, e.obs.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
                s[:], d[:] = 31, 31  # the arrays are the caller's again
                if sync:
                    torch.cuda.synchronize()
            e.step(def_act=dev[-1][0], atk_act=dev[-1][1])
        torch.cuda.synchronize()
        for n in OUTPUTS:
            assert torch.equal(getattr(engs[0], n).view(torch.uint8), getattr(engs[1], n).view(torch.uint8)), n
        sa, sb = (_live(e.export_state()) for e in engs)
        for name in sa:
            assert sa[name].tobytes() == sb[name].tobytes(), name
    finally:
        for e in engs:
            e.close()


def test_vector_env_fork():
    env = E.TDVecEnv(10, 16, "def", seed=300, autoreset=False, action_mask=True)
    try:
        env.reset()
        rng = np.random.RandomState(6)
        for _ in range(30):
            env.step(torch.from_numpy(rng.randint(0, 601, size=16).astype(np.int64)))
        obs = env.fork([0, 1], [8, 9])
        assert obs is env.engine.obs
        _assert_clones(env.engine, [0, 1], [8, 9], "fork")
        m = env._masks["def"]
        assert torch.equal(m[8], m[0]) and torch.equal(m[9], m[1])
        for _ in range(10):
            a = rng.randint(0, 601, size=16).astype(np.int64)
            a[[8, 9]] = a[[0, 1]]
            o, r, dn, info = env.step(torch.from_numpy(a))
            assert torch.equal(_rows(o, [8, 9]), _rows(o, [0, 1])) and torch.equal(_rows(r, [8, 9]), _rows(r, [0, 1]))
            assert torch.equal(info["action_mask"][8], info["action_mask"][0])
    finally:
        env.close()


def test_kernel_timing_covers_the_copy_kernel():
    """td_kernel_timing binds its next event pairs to copy kernels too (scripts/copy_bench.py)."""
    eng = _engine(10, 32, "def")
    try:
        _step(eng, _draw(np.random.RandomState(1), eng))
        eng.kernel_timing(3)
        eng.copy_boards([0, 1], [4, 5])
        _step(eng, _draw(np.random.RandomState(2), eng))
        eng.copy_boards([0], [6], write_obs=False)
        eng.copy_boards([0], [7])  # (no pair left: launched as ever)
        t = eng.kernel_times()
        assert len(t) == 3 and (t > 0).all() and (t < 1e5).all(), t
        _assert_clones(eng, [0, 1, 0], [4, 5, 7], "timed")
    finally:
        eng.close()


# ------------------------------------------------------------------ 9 kernel metadata
@pytest.mark.skipif(not (KM.TOOLS and KM.os.path.exists(KM.kernel_meta.LIB)), reason="needs the ROCm llvm tools")
def test_copy_kernel_builds_without_scratch():
    meta = KM.kernel_meta.kernels()
    for lt in (10, 20, 30, 0):
        rows = [r for n, r in meta.items() if "td_copy_kernelILi%dE" % lt in n]
        assert len(rows) == 1, (lt, sorted(meta))
        assert rows[0].get("scratch", 0) == 0, (lt, rows[0])
        opp = [r for n, r in meta.items() if "td_opponent_kernelILi%dE" % lt in n]
        assert rows[0]["lds"] <= opp[0]["lds"], (lt, rows[0], opp[0])
