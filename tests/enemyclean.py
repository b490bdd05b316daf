"""The CPU side of tests/test_gpu_enemy_clean.py: the Python restatement (oracle.td_oracle)
stepped with the seeds and actions the engines get, and what happened to each board's enemies
in each step.  Not a test module.

The step kernels mark the enemy planes of a retained observation dirty only when the step
touched an enemy (td_step_obs.h obs_dirty): one was summoned, the stable sort moved one, a
tower's shot landed, or one entered a new cell.  A step with none of the four is *quiet*: the
16 enemy planes keep their bytes, whatever became of margins, slow-down counters and
cool-downs.  The trace says, per board and step, which of the four happened, so that a run
can be refused unless every kind occurs alone often enough, and so that the marker test knows
which steps must leave a window of enemy planes unwritten."""
import numpy as np

from oracle import td_oracle as O

SUMMON, SORT, SHOT, MOVE = 1, 2, 4, 8
ENEMY = 16   # an enemy on the board after the step's actions (so: in TDBoard.step)
ENDED = 32   # the episode ended in this step (the board was reset behind it)
SLOW = 64    # a slow-down counter ran down in this step
PLANES = 128  # a byte of the 16 enemy planes differs from the step before
TOUCH = SUMMON | SORT | SHOT | MOVE

LAYOUT_RETRIES = 64   # td_kernels.h kLayoutRetries
ROAD_ATTEMPTS = 1000  # td_kernels.h kRoadAttempts
MODES = {"def": O.MODE_DEF, "atk": O.MODE_ATK, "2p": O.MODE_2P}

# The recipe of tests/test_gpu_obs_retain.py: 40-step episodes, enemies that cross a board
# side in 10-25 steps, both sides richer than the defaults.
EP = 40


def oracle_cfg(L):
    return O.Config(enemy_speed=[[.1 * L] * 2, [.05 * L] * 2, [.04 * L] * 2, [.04 * L] * 2],
                    attacker_init_cost=30, defender_init_cost=30, defender_cost_rate=1.)


def oracle_hp(multi):
    hp = O.Hyper(allow_multiple_actions=bool(multi))
    hp.max_episode_steps = EP
    return hp


def draw_actions(rng, L, n, mode, multi):
    """tests/test_gpu_obs_retain.py _actions, on the host."""
    d = a = None
    if mode != "atk":
        d = (rng.random_sample((n, 6, L, L)) < 0.01).astype(np.int64) if multi else \
            rng.randint(0, 6 * L * L + 1, size=n).astype(np.int64)
    if mode != "def":
        a = rng.randint(0, 5, size=(n, 3, 8)).astype(np.int64)
    return d, a


class _Watch(object):
    """While active, every TDBoard.step of the restatement leaves its events in ``last``."""

    def __enter__(self):
        self.step0 = O.Board.step
        self.states0 = O.Board.get_states
        watch = self

        def step(board):
            pre = list(board.enemies)  # after the actions, before the sort
            ev = ENEMY if pre else 0
            if len(pre) > board.n_before:
                ev |= SUMMON
            order = sorted(pre, key=lambda e: e.dist - e.margin)
            if any(x is not y for x, y in zip(order, pre)):
                ev |= SORT
            snap = [(e, e.LP, tuple(e.loc), e.slowdown) for e in pre]
            planes = board.enemy_LP.copy()
            reward = watch.step0(board)
            if not np.array_equal(planes.view(np.uint32), board.enemy_LP.view(np.uint32)):
                ev |= PLANES
            for e, lp, loc, slow in snap:
                if e.LP != lp:
                    ev |= SHOT
                if tuple(e.loc) != loc:
                    ev |= MOVE
                if e.slowdown < slow:
                    ev |= SLOW
            watch.last = ev
            return reward

        O.Board.step = step
        O.Board.get_states = lambda board: None  # (the trace reads no observation)
        return self

    def __exit__(self, *exc):
        O.Board.step = self.step0
        O.Board.get_states = self.states0


def _reset(env):
    for _ in range(LAYOUT_RETRIES + 1):
        try:
            env.reset()
            return
        except O.RoadGenError:
            pass
    raise AssertionError("no layout in %d draws" % (LAYOUT_RETRIES + 1))


class Trace(object):
    """``B`` boards from ``seed0`` (the first seeds whose first layout draw succeeds), ``steps``
    steps of uniform random actions from RandomState(``act_seed``), auto-reset on.

    ``cfg`` / ``hp``: another recipe than this file's (scripts/obs_delta_bytes.py: the defaults).

    seeds [B]; def_act / atk_act: per step the action arrays (or None); ev [steps, B] uint8 the
    event bits above; done [steps, B]; n_en [steps, B] the enemies after the step (before the
    reset of a finished board)."""

    def __init__(self, L, B, mode="def", multi=False, steps=300, seed0=7300, act_seed=11, cfg=None, hp=None):
        self.L, self.B, self.mode, self.multi, self.steps = L, B, mode, multi, steps
        cfg, hp = cfg or oracle_cfg(L), hp or oracle_hp(multi)
        with _Watch() as w:
            self.seeds, envs = [], []
            s = seed0
            while len(envs) < B:
                try:
                    envs.append(O.Env(L, MODES[mode], 1, s, s, cfg, hp, road_attempts=ROAD_ATTEMPTS))
                    self.seeds.append(s)
                except O.RoadGenError:
                    pass
                s += 1
            rng = np.random.RandomState(act_seed)
            self.def_act, self.atk_act = [], []
            self.ev = np.zeros((steps, B), dtype=np.uint8)
            self.done = np.zeros((steps, B), dtype=bool)
            self.n_en = np.zeros((steps, B), dtype=np.int32)
            for k in range(steps):
                d, a = draw_actions(rng, L, B, mode, multi)
                self.def_act.append(d)
                self.atk_act.append(a)
                for b, env in enumerate(envs):
                    env._board.n_before = len(env._board.enemies)
                    _, _, done, _ = env.step(None if d is None else (d[b] if multi else int(d[b])),
                                             None if a is None else a[b])
                    self.ev[k, b] = w.last | (ENDED if done else 0)
                    self.done[k, b] = done
                    self.n_en[k, b] = len(env._board.enemies)
                    if done:
                        _reset(env)
        self.seeds = np.asarray(self.seeds, dtype=np.int64)

    def kept(self):
        """[steps, B]: the board kept its episode in this step (a reset rewrites everything)."""
        return (self.ev & ENDED) == 0

    def quiet(self):
        """[steps, B]: an enemy on the board, the episode kept, and nothing touched an enemy."""
        return self.kept() & ((self.ev & ENEMY) != 0) & ((self.ev & TOUCH) == 0)

    def counts(self):
        ev, kept = self.ev, self.kept()
        alone = lambda bit: int((kept & ((ev & TOUCH) == bit)).sum())
        q = self.quiet()
        with_enemy = kept & ((ev & ENEMY) != 0)
        return {"summon": alone(SUMMON), "sort": alone(SORT), "shot": alone(SHOT), "move": alone(MOVE),
                "quiet": int(q.sum()), "quiet_slow": int((q & ((ev & SLOW) != 0)).sum()),
                "with_enemy": int(with_enemy.sum()), "planes_same": int((with_enemy & ((ev & PLANES) == 0)).sum()),
                "missed": int((kept & ((ev & TOUCH) == 0) & ((ev & PLANES) != 0)).sum())}

    def check(self):
        """The floors a run needs (raises AssertionError): each kind of event alone on at least
        20 kept board-steps (the sort: 3), 20 quiet steps with an enemy present -- in every one of
        which a margin changed -- one of them with a slow-down counter running down; and no step
        without an event changed a byte of the enemy planes."""
        c = self.counts()
        assert c["missed"] == 0, c
        assert min(c["summon"], c["shot"], c["move"], c["quiet"]) >= 20, c
        assert c["sort"] >= 3, c
        assert c["quiet_slow"] >= 1, c
        return c
