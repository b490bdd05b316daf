"""TDEngine: B independent gym-TD boards in HBM, stepped by libtdstep.so.

The batched counterpart of TDGymBasic + TDDefense / TDAttack / TDMulti
(gym_TD/envs/TDGymBasic.py, TDDefense.py, TDAttack.py, TDMulti.py).  Actions and
outputs are torch tensors on the engine's device; every step is one kernel
launch on torch's current stream.
"""
import copy
import os
import types

import numpy as np
import torch

from . import _lib
from . import params as P
from . import sampling

MODES = {"def": 0, "atk": 1, "2p": 2}

HDR_DTYPE = np.dtype([
    ("cost_def", "<f8"), ("cost_atk", "<f8"), ("ep_return", "<f8"), ("steps", "<i4"), ("base_LP", "<i4"),
    ("atk_cd", "<i4"), ("def_cd", "<i4"), ("n_en", "<i4"), ("n_tw", "<i4"), ("num_roads", "<i4"),
    ("end_cell", "<i4"), ("start_cell", "<i4", (3,)), ("maxdist", "<i4"), ("flags", "<i4"), ("episodes", "<i4"),
    ("max_cost", "<f8"), ("max_base_LP", "<i4"), ("format", "<i4")])
assert HDR_DTYPE.itemsize == _lib.HDR_BYTES


class _DeviceBlock(object):
    """A td_alloc_device block seen by torch through __cuda_array_interface__.  The
    tensor keeps this object alive; the block is freed when the last tensor (or view)
    using it is gone."""

    def __init__(self, ptr, shape, typestr):
        self.ptr = ptr
        self.__cuda_array_interface__ = {"shape": tuple(int(n) for n in shape), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 2, "strides": None}

    def __del__(self):
        try:
            if self.ptr:
                _lib.lib.td_free_device(self.ptr)
                self.ptr = None
        except Exception:  # (interpreter shutdown)
            pass


_TYPESTR = {torch.float32: "<f4", torch.float16: "<f2", torch.int64: "<i8"}
# observation dtype -> enum td_obs_format (td_set_obs_format)
OBS_FORMATS = {torch.float32: _lib.OBS_F32, torch.float16: _lib.OBS_F16}


# The engine's observation in physically contiguous device memory or a plain allocation.
# auto (default): contiguous from CONTIG_OBS_MIN bytes on -- faster there (32,768 boards at
# 10x10, 590 MB: 112.5 vs 115.5 us; 30x30 / 16,384, 2.65 GB: 498.7 vs 517.6; 65,536 +-0),
# slower below (16,384 / 8,192 / 4,096 boards: +0.6-2.2 %), profiles/r04/s26.
# TD_CONTIG_OBS=1 / 0 (or true / false, yes / no, on / off) forces it; any other value
# warns once and keeps auto.
CONTIG_OBS_MIN = 512 << 20


def _parse_contig_obs(v):
    v = (v or "auto").strip().lower()
    if v in ("1", "true", "yes", "on"):
        return True
    if v in ("0", "false", "no", "off"):
        return False
    if v != "auto":
        import warnings
        warnings.warn("TD_CONTIG_OBS=%r is not auto / 0 / 1 / true / false: using auto" % v, RuntimeWarning)
    return "auto"


CONTIG_OBS = _parse_contig_obs(os.environ.get("TD_CONTIG_OBS"))


def _contig_obs(nbytes):
    if CONTIG_OBS == "auto":
        return nbytes >= CONTIG_OBS_MIN
    return CONTIG_OBS


# The engine's device observation is retained (td_retain_obs): a step writes only the
# windows of a board's observation that may have changed since the step before.
# TD_RETAIN_OBS=0 (or false / no / off) is the A/B switch: every engine writes every byte,
# whatever its retain_obs argument; 1 / unset leaves the argument in charge; any other
# value warns once and does the same.
def _parse_retain_obs(v):
    v = (v or "1").strip().lower()
    if v in ("0", "false", "no", "off"):
        return False
    if v not in ("1", "true", "yes", "on"):
        import warnings
        warnings.warn("TD_RETAIN_OBS=%r is not 0 / 1 / true / false: using 1" % v, RuntimeWarning)
    return True


RETAIN_OBS = _parse_retain_obs(os.environ.get("TD_RETAIN_OBS"))


def device_zeros(shape, dtype, device, contiguous=None):
    """A zeroed device tensor in td_alloc_device memory (contiguous: physically contiguous
    where the driver can give it); torch.zeros if torch cannot adopt the block."""
    dev = torch.device(device)
    n = int(np.prod(shape)) * torch.tensor([], dtype=dtype).element_size()
    p = _lib.ctypes.c_void_p()
    contig = _contig_obs(n) if contiguous is None else bool(contiguous)
    if _lib.lib.td_alloc_device(n, dev.index or 0, int(contig), _lib.ctypes.byref(p)) != 0 or not p.value:
        return torch.zeros(shape, dtype=dtype, device=dev)
    blk = _DeviceBlock(p.value, shape, _TYPESTR[dtype])
    try:
        t = torch.as_tensor(blk, device=dev)
    except Exception:
        t = None
    if t is None or t.data_ptr() != p.value or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        del blk  # (frees the block)
        return torch.zeros(shape, dtype=dtype, device=dev)
    t._td_block = True  # (tests: the block was adopted)
    # how the block was placed (a refused contiguous request is a plain allocation):
    # TDEngine.obs_alloc, by which bench.py keys its PMC traffic records
    t._td_contig = _lib.lib.td_alloc_is_contiguous(p.value) == 1
    return t


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class TDEngine(object):
    """B boards of one map size and mode.

    mode: 'def' (TD-def: defender acts, built-in random_enemy_lv{difficulty}),
          'atk' (TD-atk: attacker acts, built-in random_tower_lv{difficulty}),
          '2p'  (TD-2p: both act).
    multi_action: HyperParameters.allow_multiple_actions (defender flags (6, L, L)).
    np_seeds / py_seeds: per-board seeds of the layout stream (numpy RandomState)
          and of the built-in opponent's CPython ``random`` stream.
    autoreset: a board that finishes starts its next episode inside the same
          step and the returned obs is the new episode's first obs (gym 0.21
          AsyncVectorEnv semantics); reward/done/info describe the finished step.
    host_io: step inputs and outputs live in pinned host memory that the kernels
          read and write directly (zero-copy).  For the single-env classes: one
          launch and one stream synchronisation per step, no per-tensor copies.
          A host_io step() is synchronous: it returns once the kernel has read the
          staged actions and written the outputs.
    random_agent: TDGymBasic's random_agent (False: the built-in opponent draws from
          each board's layout stream; with auto-reset the next layout is then drawn
          right after the step that ends the episode, in stream order).
    step_kernel: 'auto' (td_create's rule by batch size), 'large', 'small' or 'small2'
          (td_set_step_kernel; the three give the same results).  'auto' chooses per
          launch: a step that skips clean windows of the retained observation may run
          another kernel than one that writes every window (retained_step_kernel); a
          forced kind runs for every launch.
    obs_dtype: torch.float32 (default) or torch.float16: the element of ``obs``.  The
          float16 observation is the float32 one rounded to nearest-even, written by the
          step kernels themselves (td_set_obs_format): half the step's store stream and
          half the policy's read stream.  Everything else is unchanged ('auto' may pick
          another step kernel for the narrower stream; the results do not depend on it).
    retain_obs: True (default): the engine's device observation is retained
          (td_retain_obs) -- a step leaves unwritten what its previous step already left
          there, so ``obs`` must only be read: code that writes into the tensor ``step``
          returns (in-place normalisation, masking) must work on a copy, or construct
          with retain_obs=False.  Ignored with host_io; TD_RETAIN_OBS=0 turns it off
          for every engine.
    frame_skip: board steps per ``step()`` (td_set_frame_skip), 1 (default) .. 16.  With
          k > 1 a step is a macro step: the given action, then k - 1 empty actions, in one
          launch that writes one observation; reward is the sum, done / info those of the
          last board step run (a board stops at its episode's end), RealAction / FailCode
          those of the first.  Discrete actions and random_agent=True only.
    sample_seed: the seed of ``sample_actions`` (an int in [0, 2**64), default 0): its draws
          are a function of this seed, the call's ticket and the board id, and of nothing else.
    """

    def __init__(self, map_size, n_boards, mode="def", multi_action=None, difficulty=1, device=None,
                 np_seeds=None, py_seeds=None, autoreset=True, info=True, cfg=None, hp=None, host_io=False,
                 random_agent=True, step_kernel="auto", obs_dtype=torch.float32, retain_obs=True, frame_skip=1,
                 sample_seed=0):
        frame_skip = _check_frame_skip(frame_skip)  # (before td_create: no device is touched)
        if isinstance(sample_seed, (bool, np.bool_)) or not isinstance(sample_seed, (int, np.integer)) or \
                not 0 <= int(sample_seed) <= sampling.M64:
            raise ValueError("sample_seed must be an int in [0, 2**64), not %r" % (sample_seed,))
        self.sample_seed, self._sample_ticket = int(sample_seed), 0
        # state serial: advanced by every call that can change a board or the config (_changed);
        # _mask_at: the serial at which the mask / code buffers were last written whole
        self._state_serial, self._mask_at, self._mask_pending = 0, {}, None
        if obs_dtype not in OBS_FORMATS:  # (before td_create: no device is touched)
            raise ValueError("obs_dtype must be torch.float32 or torch.float16, not %r" % (obs_dtype,))
        if not isinstance(retain_obs, (bool, np.bool_)):
            raise ValueError("retain_obs must be True or False, not %r" % (retain_obs,))
        self.obs_dtype = obs_dtype
        self.retain_obs = bool(retain_obs) and RETAIN_OBS and not host_io
        hp = hp or P.hyper_parameters
        if multi_action is None:
            multi_action = bool(hp.allow_multiple_actions)
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.L, self.B, self.mode = int(map_size), int(n_boards), mode
        self.multi = bool(multi_action)
        self.difficulty = int(difficulty)
        self._cfg_c = P.to_c(cfg or P.config, hp)
        self._cfg_hist = {0: copy.deepcopy(cfg or P.config)}  # paramConfig epoch -> config (td_config_epoch)
        h = _lib.lib.td_create(self._cfg_c, self.L, self.B, MODES[mode], int(self.multi), self.difficulty,
                               self.device.index or 0)
        if not h:
            raise _lib.TDError(_lib.lib.td_last_error().decode())
        self._h = h
        self.lw = _lib.lib.td_layout_words(self.L)
        self.autoreset = bool(autoreset)
        _lib.check(_lib.lib.td_set_autoreset(h, int(self.autoreset)))
        self.random_agent = bool(random_agent)
        if not self.random_agent:  # opponents on the layout stream (needs auto-reset off)
            _lib.check(_lib.lib.td_set_random_agent(h, 0))
        B, L = self.B, self.L
        self.host_io = bool(host_io)
        dev = torch.device("cpu") if self.host_io else self.device
        zeros = (lambda shape, dtype: torch.zeros(shape, dtype=dtype).pin_memory()) if self.host_io else \
            (lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev))
        # the observation, the step's write stream: contiguous device memory (td_alloc_device)
        self.obs = zeros((B, _lib.NCH, L, L), obs_dtype) if self.host_io else \
            device_zeros((B, _lib.NCH, L, L), obs_dtype, self.device)
        if obs_dtype != torch.float32:
            _lib.check(_lib.lib.td_set_obs_format(h, OBS_FORMATS[obs_dtype]))
        assert _lib.lib.td_obs_bytes(h) == self.obs.numel() * self.obs.element_size()
        self._arm_retain(True)
        # how the observation was allocated (bench.py keys PMC traffic records by it)
        self.obs_alloc = "host" if self.host_io else "contiguous" if getattr(self.obs, "_td_contig", False) else "plain"
        self.reward = zeros(B, torch.float64)
        self.done = zeros(B, torch.uint8)
        self.info_enabled = bool(info)
        self.win = self.allow_next = self.cooldowns = self.ep_return = self.ep_len = None
        self.real_def = self.fail_def = self.real_atk = self.fail_atk = None
        if info:
            self.win = zeros(B, torch.int8)
            self.allow_next = zeros(B, torch.uint8)
            self.cooldowns = zeros(B, torch.uint8)
            self.ep_return = zeros(B, torch.float64)
            self.ep_len = zeros(B, torch.int32)
            if mode != "atk":
                shape = (B, 6, L, L) if self.multi else (B,)
                self.real_def = zeros(shape, torch.int64) if self.host_io or not self.multi else \
                    device_zeros(shape, torch.int64, self.device)
                self.fail_def = zeros(B, torch.int32)
            if mode != "def":
                self.real_atk = zeros((B, 3, 8), torch.int64)
                self.fail_atk = zeros((B, 3), torch.int32)
        if self.host_io:  # action staging, read by the kernel from pinned host memory
            self._def_in = zeros((B, 6, L, L) if self.multi else (B,), torch.int64) if mode != "atk" else None
            self._atk_in = zeros((B, 3, 8), torch.int64) if mode != "def" else None
        self._io = _lib.TdStepIO()
        # host_io: numpy views of the pinned buffers, made once (a torch -> numpy
        # conversion or a scalar read through torch costs microseconds per step)
        self.np = types.SimpleNamespace()
        for name in ("obs", "reward", "done", "real_def", "real_atk", "fail_def", "fail_atk", "win",
                     "allow_next", "cooldowns", "ep_return", "ep_len"):
            t = getattr(self, name)
            setattr(self._io, name, t.data_ptr() if t is not None else None)
            if self.host_io:
                setattr(self.np, name, t.numpy() if t is not None else None)
        if self.host_io:
            self._def_np = self._def_in.numpy() if self._def_in is not None else None
            self._atk_np = self._atk_in.numpy() if self._atk_in is not None else None
        if np_seeds is not None or py_seeds is not None:
            self.seed(np_seeds, py_seeds)
        if step_kernel != "auto":
            self.set_step_kernel(step_kernel)
        self.frame_skip = 1
        if frame_skip != 1:
            try:
                self.set_frame_skip(frame_skip)
            except Exception:
                self.close()
                raise
        P._live.add(self)

    # ------------------------------------------------------------------ setup
    def _arm_retain(self, own):
        """Retain ``self.obs`` if the engine allocated it as a td_alloc_device block (whose
        release drops the retention, so a reused address is never taken for it); a
        caller's buffer, or one torch's allocator may hand out again, is written whole."""
        if self.retain_obs:
            mine = own and getattr(self.obs, "_td_block", False)
            _lib.check(_lib.lib.td_retain_obs(self._h, self.obs.data_ptr() if mine else None))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.td_destroy(self._h)
            self._h = None
        P._live.discard(self)  # paramConfig reaches live engines only

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_config(self, cfg=None, hp=None):
        """paramConfig on this engine: the new values apply from the next step; live
        enemies and towers keep the values they were created / upgraded with, and each
        board the max_cost / base_LP of its last reset (TDElements.py:4-69, TDBoard.py:66-72)."""
        self._cfg_c = P.to_c(cfg or P.config, hp)
        self._changed()
        _lib.check(_lib.lib.td_set_config(self._h, self._cfg_c))
        self._cfg_hist[_lib.lib.td_config_epoch(self._h)] = copy.deepcopy(cfg or P.config)

    def config_of_epoch(self, ep):
        """The game config of paramConfig epoch ``ep`` (entity words carry their epoch)."""
        return self._cfg_hist.get(ep, P.config)

    def seed(self, np_seeds=None, py_seeds=None):
        """Per-board seeds (int or array of B)."""
        def arr(s):
            if s is None:
                return None
            a = np.asarray(s, dtype=np.int64)
            if a.ndim == 0:
                a = np.full(self.B, int(a), dtype=np.int64)
            if a.shape != (self.B,) or (a < 0).any() or (a > 0xFFFFFFFF).any():
                raise ValueError("seeds must be B ints in [0, 2**32)")
            return _u32(a)
        npa, pya = arr(np_seeds), arr(py_seeds)
        _lib.check(_lib.lib.td_seed(self._h, _lib.ptr(npa, _lib.ctypes.c_uint32) if npa is not None else None,
                                    _lib.ptr(pya, _lib.ctypes.c_uint32) if pya is not None else None))

    def set_py_state(self, b, state):
        """Import a CPython ``random.getstate()`` (or 625 words) as board b's opponent stream."""
        w = _mt_words(state)
        _lib.check(_lib.lib.td_set_py_state(self._h, int(b), _lib.ptr(w, _lib.ctypes.c_uint32)))

    def get_py_state(self, b):
        w = np.zeros(_lib.MT_WORDS, dtype=np.uint32)
        _lib.check(_lib.lib.td_get_py_state(self._h, int(b), _lib.ptr(w, _lib.ctypes.c_uint32)))
        return w

    def set_np_state(self, b, state):
        """Import a ``RandomState.get_state()`` (or 625 words) as board b's layout stream."""
        w = _mt_words(state)
        _lib.check(_lib.lib.td_set_np_state(self._h, int(b), _lib.ptr(w, _lib.ctypes.c_uint32)))

    def get_np_state(self, b):
        w = np.zeros(_lib.MT_WORDS, dtype=np.uint32)
        _lib.check(_lib.lib.td_get_np_state(self._h, int(b), _lib.ptr(w, _lib.ctypes.c_uint32)))
        return w

    # ------------------------------------------------------------------- run
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def reset(self, mask=None):
        """TDGymBasic.reset for the boards in ``mask`` (None = all).  Returns the
        obs tensor (B, 45, L, L) and the list of boards whose road generation
        failed (the reference raises or hangs there; those boards are unchanged)."""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint8).reshape(self.B))
        torch.cuda.synchronize(self.device)
        self._changed()
        rc = _lib.lib.td_reset(self._h, _lib.ptr(m, _lib.ctypes.c_uint8) if m is not None else None,
                               self.obs.data_ptr(), self._stream())
        _lib.check(rc)
        failed = []
        if rc > 0:
            ids = np.zeros(rc, dtype=np.int32)
            _lib.lib.td_last_reset_failures(self._h, _lib.ptr(ids, _lib.ctypes.c_int32), rc)
            failed = ids.tolist()
        return self.obs, failed

    def reset_all(self, max_retries=64):
        """reset() every board, redrawing (from the same streams) the layouts whose
        road generation failed -- the reference would raise or hang on those draws
        (TDRoadGen.py:177-189).  Returns (obs, number of failed draws skipped)."""
        obs, failed = self.reset()
        skipped = 0
        while failed and max_retries > 0:
            skipped += len(failed)
            m = np.zeros(self.B, dtype=np.uint8)
            m[failed] = 1
            obs, failed = self.reset(m)
            max_retries -= 1
        if failed:
            raise RuntimeError("road generation kept failing for boards %r" % failed[:8])
        return obs, skipped

    def reset_layouts(self, recs, boards):
        recs = _u32(recs).reshape(-1, self.lw)
        ids = np.ascontiguousarray(boards, dtype=np.int32)
        torch.cuda.synchronize(self.device)
        self._changed()
        _lib.check(_lib.lib.td_reset_layouts(self._h, _lib.ptr(recs, _lib.ctypes.c_uint32),
                                             _lib.ptr(ids, _lib.ctypes.c_int32), len(ids), self.obs.data_ptr(),
                                             self._stream()))
        return self.obs

    def step(self, def_act=None, atk_act=None):
        """One step of every board; returns (obs, reward, done) device tensors.

        The tensors are the engine's own buffers, overwritten by the next step
        (clone them to keep a history).  The returned obs tensor is the engine's buffer:
        read it, do not write it -- with retain_obs (the default) the next step leaves
        unwritten whatever it knows its last write left there."""
        return self._launch_step(def_act, atk_act)

    def step_boards(self, boards, def_act=None, atk_act=None):
        """One step of the boards named in ``boards`` only (td_step_boards): exactly the step
        ``step()`` would have given each of them, while every other board keeps its state, its
        streams and its rows of every output tensor -- with ``copy_boards`` the loop of a
        search: fork the leaves, step the leaves, read their rows.  The reference's
        counterpart is ``child.step(a)`` on the env objects one chooses.

        ``boards``: board ids as an int sequence, numpy array or tensor (``copy_boards``' rules:
        a GPU tensor is brought to the host first; int32 numpy arrays are taken as they are),
        in any order, none twice.  The actions are full-batch tensors of the shapes ``step()``
        checks; only the rows of the named boards are read.  Returns (obs, reward, done), the
        engine's own full tensors with only the named rows fresh; the info tensors likewise.

        One kernel on torch's current stream, which must be the stream of step(); nothing is
        synchronised (with ``host_io`` the call waits for the kernel, as ``step()`` does).  An
        empty list is a no-op.  TDError, with nothing changed: an id out of range or named
        twice, ``frame_skip`` > 1, random_agent=False with auto-reset on.
        Ids that are on the device already: ``step_boards_dev`` (no copy to the host, no wait)."""
        return self._launch_step(def_act, atk_act, _board_ids(boards))

    def step_boards_dev(self, boards, def_act=None, atk_act=None, count=None, status=None):
        """``step_boards`` for ids that are on the device (td_step_boards_dev): nothing is copied
        to the host and nothing is waited for -- the list is validated by a kernel on the
        stream, in front of the step's.

        ``boards``: an integer tensor on the engine's device (int32 and contiguous is taken as
        it is, any other integer tensor is converted on the device); its length is the call's
        ``cap``.  A CPU tensor, list or numpy array raises ValueError: that is ``step_boards``.
        ``count``: None (every entry is used) or a one-element int32 device tensor: the first
        ``count[0]`` entries are used, the rest is never read as ids -- compact "the boards
        that are not done" into a buffer of fixed size and pass its length here.
        ``status``: an optional int32 device tensor of 4 elements, receives the call's verdict
        (code, call, entry, board; code 0 = accepted) in stream order.

        A list the device refuses (a count outside [0, cap], an id out of range, a board named
        twice) changes nothing at all; ``list_errors()`` tells afterwards.  TDError at once, with
        nothing changed: more ids than boards, ``frame_skip`` > 1, random_agent=False with
        auto-reset on.  With ``retain_obs`` clean windows are skipped only while every board's
        row is known.  The tensors stay alive until the next call; with ``host_io`` the call
        waits for the kernel, as ``step()`` does.  Returns (obs, reward, done)."""
        ids = _dev_ids(boards, self.device, "step_boards")
        dev = (ids, _dev_words(count, 1, self.device, "count"), _dev_words(status, 4, self.device, "status"))
        return self._launch_step(def_act, atk_act, None, dev)

    def _call_step(self, io, ids, dev):
        if dev is not None:
            b, c, st = dev
            self._changed(("dev", b, c))
            return _lib.lib.td_step_boards_dev(self._h, io, b.data_ptr(), int(b.numel()),
                                               c.data_ptr() if c is not None else None,
                                               st.data_ptr() if st is not None else None, self._stream())
        if ids is None:
            self._changed()
            return _lib.lib.td_step(self._h, io, self._stream())
        self._changed(("host", ids.copy()))
        return _lib.lib.td_step_boards(self._h, io, ids.ctypes.data, int(ids.size), self._stream())

    def _launch_step(self, def_act, atk_act, ids=None, dev=None):
        """step() (ids None), step_boards() or step_boards_dev() (dev: the id, count and status
        tensors): stage the actions, launch, hand out the tensors."""
        io = self._io
        keep = [t for t in dev if t is not None] if dev is not None else []
        if self.host_io:
            if self.mode != "atk":
                self._def_np[...] = np.asarray(def_act, dtype=np.int64).reshape(self._def_np.shape)
                io.def_act = self._def_in.data_ptr()
            if self.mode != "def":
                self._atk_np[...] = np.asarray(atk_act, dtype=np.int64).reshape(self._atk_np.shape)
                io.atk_act = self._atk_in.data_ptr()
            _lib.check(self._call_step(io, ids, dev))
            # the outputs are the caller's as soon as this returns, and the next call
            # rewrites the staged actions: wait for the kernel
            torch.cuda.current_stream(self.device).synchronize()
            return self.obs, self.reward, self.done
        if self.mode != "atk":
            d = _as_dev(def_act, torch.int64, self.device)
            exp = (self.B, 6, self.L, self.L) if self.multi else (self.B,)
            if tuple(d.shape) != exp:
                raise ValueError("defender action must have shape %r" % (exp,))
            keep.append(d)
            io.def_act = d.data_ptr()
        if self.mode != "def":
            a = _as_dev(atk_act, torch.int64, self.device)
            if tuple(a.shape) != (self.B, 3, 8):
                raise ValueError("attacker action must have shape (B, 3, 8)")
            keep.append(a)
            io.atk_act = a.data_ptr()
        _lib.check(self._call_step(io, ids, dev))
        self._keep = keep  # actions (and a device list) stay alive until the next call
        return self.obs, self.reward, self.done

    def copy_boards(self, src, dst, write_obs=True):
        """Make boards ``dst[i]`` exact copies of boards ``src[i]`` on the device
        (td_copy_boards): the fork of a search -- one root repeated in ``src`` gives many
        children.  The reference's counterpart is ``copy.deepcopy(env)``.

        ``src`` / ``dst``: equally many board ids as int sequences, numpy arrays or tensors; a
        GPU tensor is brought to the host first (a device-to-host copy that waits for that
        tensor), so pass host ids where the call must not wait; int32 numpy arrays are taken as
        they are, anything else is converted (O(n) on the host, as the library's check of the
        ids is).  No board may be named twice
        in ``dst`` or in both (TDError, nothing changes).  Header, live enemies and towers with
        their config epochs, cells and the opponent's stream are copied; with
        random_agent=True each destination keeps its own layout sequence for its next
        episodes, with random_agent=False the shared numpy stream is copied too.

        One kernel on torch's current stream, which must be the stream of step(); nothing is
        synchronised.  With ``write_obs`` the destinations' observations are written whole
        into ``self.obs`` (the rows of the sources' present states); without it nothing is
        written and the next step writes every byte.  The engine's other last-step tensors
        (``reward``, ``done``, the info tensors) keep ``dst``'s old rows until the next step.
        Returns ``self.obs``.
        Ids that are on the device already: ``copy_boards_dev`` (no copy to the host, no wait)."""
        s, d = _board_ids(src), _board_ids(dst)
        if s.shape != d.shape:
            raise ValueError("src and dst must name equally many boards, got %d and %d" % (s.size, d.size))
        self._changed(("host", d.copy()))
        _lib.check(_lib.lib.td_copy_boards(self._h, s.ctypes.data, d.ctypes.data, int(s.size),
                                           self.obs.data_ptr() if write_obs else None, self._stream()))
        return self.obs

    def copy_boards_dev(self, src, dst, count=None, write_obs=True, status=None):
        """``copy_boards`` for ids that are on the device (td_copy_boards_dev): nothing is copied
        to the host and nothing is waited for; the lists are validated by a kernel on the
        stream, in front of the copy's.

        ``src`` / ``dst``: integer tensors of one length on the engine's device (int32 and
        contiguous is taken as it is); ``count`` and ``status`` as in ``step_boards_dev``.  A CPU
        tensor, list or numpy array raises ValueError: that is ``copy_boards``.  A list the
        device refuses (a bad count, an id out of range, a board twice in ``dst`` or in both)
        changes nothing; ``list_errors()`` tells afterwards.  The tensors stay alive until the
        next call.  Returns ``self.obs``."""
        s = _dev_ids(src, self.device, "copy_boards")
        d = _dev_ids(dst, self.device, "copy_boards")
        if s.numel() != d.numel():
            raise ValueError("src and dst must name equally many boards, got %d and %d" % (s.numel(), d.numel()))
        c = _dev_words(count, 1, self.device, "count")
        st = _dev_words(status, 4, self.device, "status")
        self._changed(("dev", d, c))
        _lib.check(_lib.lib.td_copy_boards_dev(self._h, s.data_ptr(), d.data_ptr(), int(s.numel()),
                                               c.data_ptr() if c is not None else None,
                                               self.obs.data_ptr() if write_obs else None,
                                               st.data_ptr() if st is not None else None, self._stream()))
        self._keep_list = (s, d, c, st)  # alive until the next call's kernels are behind them on the stream
        if self.host_io:
            torch.cuda.current_stream(self.device).synchronize()
        return self.obs

    def list_errors(self, clear=True):
        """Device-list calls (``step_boards_dev``, ``copy_boards_dev``, ``action_mask_boards_dev``) whose list the device
        refused since the last clear (td_list_errors; waits for the device): ``(n_refused,
        first)``, ``first`` None or a dict with ``code`` (1 count, 2 range, 3 twice, 4 overlap),
        ``call`` (the call's serial), ``entry`` and ``board``."""
        rec = _lib.TdListStatus()
        n = _lib.check(_lib.lib.td_list_errors(self._h, _lib.ctypes.byref(rec), int(bool(clear))))
        first = dict(code=rec.code, call=rec.call, entry=rec.entry, board=rec.board) if n else None
        return n, first

    def step_boards_dev_kernel_name(self):
        """The kernel ``step_boards_dev`` launches behind its check (td_step_boards_dev_kernel_name)."""
        return _lib.lib.td_step_boards_dev_kernel_name(self._h).decode()

    def _mask_prepare(self, code):
        """The engine's mask buffers (allocated on first use) as a td_mask_io."""
        B, L = self.B, self.L
        io = getattr(self, "_mask_io", None)
        if io is None:
            io = self._mask_io = _lib.TdMaskIO()
            self._mask_buf = {}
            if self.mode != "atk":
                if self.multi:
                    self._mask_pitch, shape = 0, (B, 6, L, L)
                else:
                    self._mask_pitch = (6 * L * L + 1 + 15) & ~15
                    shape = (B, self._mask_pitch)
                self._mask_shape = shape
                self._mask_buf["def"] = torch.zeros(shape, dtype=torch.uint8, device=self.device)
                io.def_mask = self._mask_buf["def"].data_ptr()
                io.def_pitch = self._mask_pitch
            if self.mode != "def":
                self._mask_buf["atk"] = torch.zeros((B, 3, 5), dtype=torch.uint8, device=self.device)
                io.atk_mask = self._mask_buf["atk"].data_ptr()
        if code and self.mode != "atk" and "def_code" not in self._mask_buf:
            self._mask_buf["def_code"] = torch.zeros(self._mask_shape, dtype=torch.uint8, device=self.device)
        io.def_code = self._mask_buf["def_code"].data_ptr() if code and self.mode != "atk" else None
        return io

    def _mask_views(self, code):
        A = 6 * self.L * self.L + 1
        out = {}
        for k, t in self._mask_buf.items():
            if k == "def_code" and not code:
                continue
            out[k] = t[:, :A] if k != "atk" and not self.multi else t
        return out

    def action_mask(self, code=False):
        """Legal-action masks of every board's present state (td_action_mask): what the next
        step() would execute if the action were the only thing asked of that side.

        Returns a dict of uint8 device tensors, by mode: ``"def"`` (B, 6 L^2 + 1), the
        no-op last -- or (B, 6, L, L) with multi-action, each flag on its own --,
        ``"def_code"`` (with ``code``: the fail code each operation would return, the
        cool-down aside) and ``"atk"`` (B, 3, 5), type 4 = none.  One kernel on torch's
        current stream, which must be the stream of step().  The tensors are the engine's
        own buffers (allocated on first use, overwritten by the next call); the discrete
        defender rows are padded to a multiple of 16 bytes, the returned tensor is the
        view without the padding."""
        io = self._mask_prepare(code)
        _lib.check(_lib.lib.td_action_mask(self._h, io, self._stream()))
        # every row of the buffers written describes the present state (refresh_action_mask)
        self._mask_at["mask"] = self._state_serial
        if code and self.mode != "atk":
            self._mask_at["code"] = self._state_serial
        return self._mask_views(code)

    def action_mask_boards(self, boards, code=False):
        """``action_mask`` for the boards named in ``boards`` only (td_action_mask_boards): with
        ``copy_boards`` and ``step_boards`` the third call of a search iteration -- fork the
        leaves, step the leaves, mask the leaves -- at the cost of the leaves.

        ``boards``: board ids under ``step_boards``' rules (int sequence, numpy array or tensor;
        a GPU tensor is brought to the host first), any order, none twice.  Writes into the
        engine's own mask buffers, the ones ``action_mask()`` returns (allocated on first use),
        and returns the same dict of full tensors: only the named rows are fresh, every other
        row keeps the bytes it had, whatever state they describe.  One kernel on torch's
        current stream, which must be the stream of step(); nothing is synchronised, no board
        changes.  An empty list is a no-op.  TDError, nothing written: an id out of range or
        named twice.  ``frame_skip`` > 1 and random_agent=False are fine here.
        Ids that are on the device already: ``action_mask_boards_dev``."""
        ids = _board_ids(boards)
        io = self._mask_prepare(code)
        _lib.check(_lib.lib.td_action_mask_boards(self._h, io, ids.ctypes.data, int(ids.size), self._stream()))
        return self._mask_views(code)

    def action_mask_boards_dev(self, boards, count=None, status=None, code=False):
        """``action_mask_boards`` for ids that are on the device (td_action_mask_boards_dev):
        nothing is copied to the host and nothing is waited for; the list is validated by a
        kernel on the stream, in front of the mask's.

        ``boards``, ``count`` and ``status`` as in ``step_boards_dev`` (a CPU tensor, list or
        numpy array raises ValueError: that is ``action_mask_boards``).  A list the device
        refuses (a count outside [0, cap], an id out of range, a board named twice) writes no
        byte; ``list_errors()`` tells afterwards.  Returns the engine's full mask tensors:
        only the named rows are fresh.  The tensors stay alive until the next call."""
        ids = _dev_ids(boards, self.device, "action_mask_boards")
        c = _dev_words(count, 1, self.device, "count")
        st = _dev_words(status, 4, self.device, "status")
        io = self._mask_prepare(code)
        _lib.check(_lib.lib.td_action_mask_boards_dev(self._h, io, ids.data_ptr(), int(ids.numel()),
                                                      c.data_ptr() if c is not None else None,
                                                      st.data_ptr() if st is not None else None, self._stream()))
        self._keep_mask_list = (ids, c, st)  # alive until the next call's kernels are behind them on the stream
        return self._mask_views(code)

    def action_mask_boards_kernel_name(self):
        """The kernel ``action_mask_boards`` and ``action_mask_boards_dev`` launch
        (td_action_mask_boards_kernel_name), e.g. 'td_mask_list_kernel<10>'."""
        return _lib.lib.td_action_mask_boards_kernel_name(self._h).decode()

    # ---------------------------------------------------------------- sampling
    def _sample_prepare(self, ticket, def_idle, atk_idle, counts):
        """The engine's sample buffers (allocated on first use: every row the no-op / all-4) as a
        td_sample_io for this call's ticket."""
        B, L = self.B, self.L
        buf = getattr(self, "_sample_buf", None)
        if buf is None:
            buf = self._sample_buf = {"def": None, "atk": None, "def_count": None, "atk_count": None}
            if self.mode != "atk":
                if self.multi:
                    buf["def"] = torch.zeros((B, 6, L, L), dtype=torch.int64, device=self.device)
                else:
                    buf["def"] = torch.full((B,), 6 * L * L, dtype=torch.int64, device=self.device)
            if self.mode != "def":
                buf["atk"] = torch.full((B, 3, 8), 4, dtype=torch.int64, device=self.device)
        if counts:
            for side in ("def", "atk"):
                if buf[side] is not None and buf[side + "_count"] is None:
                    buf[side + "_count"] = torch.zeros(B, dtype=torch.int32, device=self.device)
        if ticket is None:
            ticket = self._sample_ticket
            self._sample_ticket = (ticket + 1) & sampling.M64
        io = _lib.TdSampleIO(seed=self.sample_seed, ticket=int(ticket) & sampling.M64,
                             def_idle=sampling.idle_units(def_idle), atk_idle=sampling.idle_units(atk_idle))
        for name, key in (("def_act", "def"), ("atk_act", "atk"), ("def_count", "def_count"), ("atk_count", "atk_count")):
            t = buf[key]
            setattr(io, name, t.data_ptr() if t is not None and (counts or not key.endswith("count")) else None)
        out = dict(buf)
        if not counts:
            out["def_count"] = out["atk_count"] = None
        return io, out

    def sample_actions(self, ticket=None, def_idle=0.0, atk_idle=0.0, counts=False):
        """One uniformly drawn legal action per side and board, on the device
        (td_sample_actions): what ``action_mask()`` + ``torch.multinomial`` would give, in one
        kernel and in the formats ``step()`` takes.

        Returns a dict of the engine's own device tensors (allocated on first use, overwritten
        by the next call): ``"def"`` int64 (B,) -- the no-op 6 L^2 where nothing is legal or the
        side idles -- or (B, 6, L, L) with multi-action (one flag at most), ``"atk"`` int64
        (B, 3, 8), all 4 but the chosen road's first slot, and with ``counts`` ``"def_count"`` /
        ``"atk_count"`` int32 (B,): the number of candidates (the pick's log-probability is
        -log n).  A side the mode lacks, and the counts without ``counts``, are None.
        ``def_idle`` / ``atk_idle``: the probability of choosing nothing although something is
        legal, a float in [0, 1] (an int is taken in units of 2^-32).
        The draw is a function of (``sample_seed``, ticket, board id) alone
        (gym_TD.sampling.reference_sample): ``ticket=None`` uses and then advances the engine's
        counter, an explicit ticket reproduces a call.  One candidate per side, so the step
        executes what was sampled.  No board, stream or flag changes; one kernel on torch's
        current stream, which must be the stream of step().  With ``host_io`` the tensors are
        still on the device: copy them to the host for ``step()``."""
        io, out = self._sample_prepare(ticket, def_idle, atk_idle, counts)
        _lib.check(_lib.lib.td_sample_actions(self._h, io, self._stream()))
        return out

    def sample_actions_boards(self, boards, ticket=None, def_idle=0.0, atk_idle=0.0, counts=False):
        """``sample_actions`` for the boards named in ``boards`` only (td_sample_actions_boards),
        the partner of ``step_boards``: the tensors keep their full-batch shape, only the named
        rows are written, and a named board's row is the one ``sample_actions`` gives it under
        the same ticket.  ``boards`` under ``step_boards``' rules; TDError, nothing written: an
        id out of range or named twice.  ``frame_skip`` > 1 and random_agent=False are fine."""
        ids = _board_ids(boards)
        io, out = self._sample_prepare(ticket, def_idle, atk_idle, counts)
        _lib.check(_lib.lib.td_sample_actions_boards(self._h, io, ids.ctypes.data, int(ids.size), self._stream()))
        return out

    def sample_actions_boards_dev(self, boards, count=None, status=None, ticket=None, def_idle=0.0, atk_idle=0.0,
                                  counts=False):
        """``sample_actions_boards`` for ids that are on the device (td_sample_actions_boards_dev),
        the partner of ``step_boards_dev``: nothing is copied to the host or waited for.
        ``boards``, ``count`` and ``status`` as in ``step_boards_dev``; a list the device refuses
        writes no byte (``list_errors()``).  The tensors stay alive until the next call."""
        ids = _dev_ids(boards, self.device, "sample_actions_boards")
        c = _dev_words(count, 1, self.device, "count")
        st = _dev_words(status, 4, self.device, "status")
        io, out = self._sample_prepare(ticket, def_idle, atk_idle, counts)
        _lib.check(_lib.lib.td_sample_actions_boards_dev(self._h, io, ids.data_ptr(), int(ids.numel()),
                                                         c.data_ptr() if c is not None else None,
                                                         st.data_ptr() if st is not None else None, self._stream()))
        self._keep_sample_list = (ids, c, st)  # alive until the next call's kernels are behind them on the stream
        return out

    def sample_actions_kernel_name(self):
        """The kernel the three sampling calls launch (td_sample_actions_kernel_name), e.g.
        'td_sample_kernel<10>'."""
        return _lib.lib.td_sample_actions_kernel_name(self._h).decode()

    def _sample_weighted_prepare(self, def_w, atk_w, ticket, mass):
        """The weights checked, and the engine's sample buffers (``sample_actions``' own, and the
        masses allocated on first use) as a td_sample_w_io for this call's ticket."""
        B, L = self.B, self.L
        A1 = 6 * L * L + 1

        def weights(w, name, cols, strided):
            if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.device != self.device:
                raise ValueError("%s must be a float32 tensor on %s, not %r" % (
                    name, self.device, (w.dtype, w.device) if isinstance(w, torch.Tensor) else type(w)))
            if tuple(w.shape) != (B, cols):
                raise ValueError("%s must have shape (%d, %d), not %r" % (name, B, cols, tuple(w.shape)))
            if w.stride(1) != 1 or (w.stride(0) != cols if not strided else not cols <= w.stride(0) <= 65536):
                raise ValueError("%s must be contiguous in its last dimension%s, not strides %r" % (
                    name, " with a row pitch in [%d, 65536] floats" % cols if strided else " and its rows packed", w.stride()))
            return w

        if self.multi and (self.mode == "def" or def_w is not None):
            raise ValueError("sample_weighted: the defender side is not supported with multi-action")
        want = {"def": self.mode != "atk" and not self.multi, "atk": self.mode != "def"}
        given = {"def": def_w, "atk": atk_w}
        for side in ("def", "atk"):
            if given[side] is None and want[side]:
                raise ValueError("sample_weighted: %s_w is required in mode %r" % (side, self.mode))
            if given[side] is not None and not want[side]:
                raise ValueError("sample_weighted: mode %r has no %s side (%s_w)" % (
                    self.mode, "defender" if side == "def" else "attacker", side))
        if want["def"]:
            weights(def_w, "def_w", A1, True)
        if want["atk"]:
            weights(atk_w, "atk_w", 13, False)
        self._sample_prepare(0, 0.0, 0.0, False)  # (the buffers; takes no ticket)
        buf = self._sample_buf
        if mass:
            for side in ("def", "atk"):
                if want[side] and buf.get(side + "_mass") is None:
                    buf[side + "_mass"] = torch.zeros((B, 2), dtype=torch.int64, device=self.device)
        if ticket is None:
            ticket = self._sample_ticket
            self._sample_ticket = (ticket + 1) & sampling.M64
        io = _lib.TdSampleWIO(seed=self.sample_seed, ticket=int(ticket) & sampling.M64)
        out = {"def": None, "atk": None}
        if mass:
            out["def_mass"] = out["atk_mass"] = None
        for side in ("def", "atk"):
            if not want[side]:
                continue
            setattr(io, side + "_act", buf[side].data_ptr())
            setattr(io, side + "_w", given[side].data_ptr())
            out[side] = buf[side]
            if mass:
                setattr(io, side + "_mass", buf[side + "_mass"].data_ptr())
                out[side + "_mass"] = buf[side + "_mass"]
        if want["def"]:
            io.def_w_pitch = int(def_w.stride(0))
        self._keep_sample_weights = (def_w, atk_w)  # alive until the next call's kernel is behind them on the stream
        return io, out

    def sample_weighted(self, def_w=None, atk_w=None, ticket=None, mass=False):
        """One legal action per side and board drawn in proportion to the caller's weights, on
        the device (td_sample_weighted): what ``action_mask()`` + ``w * mask`` +
        ``torch.multinomial`` + a scatter would give, in one kernel and in the formats ``step()``
        takes -- a policy network's action distribution, PUCT priors, a heuristic prior.

        ``def_w``: float32 device tensor (B, 6 L^2 + 1), the no-op last (a view with strides
        (pitch, 1), pitch <= 65,536 floats, is taken as it is); ``atk_w``: float32 (B, 13), entry
        road * 4 + type and "summon nothing" last.  Weights are meant in [0, 1] -- probabilities,
        or ``gym_TD.sampling.weights_from_logits(logits)`` --, quantised to multiples of 2^-31
        (values above 1 count as 1; NaN, negatives and values below 2^-31 as 0) and summed as
        integers over the legal entries: the result equals
        ``gym_TD.sampling.reference_sample_weighted`` bit for bit.  Nothing legal with weight:
        the no-op.  Idling is the no-op's own weight: there is no idle probability.  Each side
        the mode has needs its weights; multi-action defenders are not supported.

        Returns a dict of the engine's own device tensors, the ones ``sample_actions`` writes
        (``step_boards(..., eng._sample_buf)`` keeps working): ``"def"`` int64 (B,), ``"atk"``
        int64 (B, 3, 8), and with ``mass`` ``"def_mass"`` / ``"atk_mass"`` int64 (B, 2) =
        (m(chosen), S), (0, 0) where S == 0: the pick's log-probability is log m - log S.  A side
        the mode lacks is None.  ``sample_seed`` and the ticket counter are ``sample_actions``'
        (a weighted and a uniform call at one ticket share random words: leave ``ticket=None``
        or vary it).  No board, stream or flag changes; one kernel on torch's current stream,
        which must be the stream of step()."""
        io, out = self._sample_weighted_prepare(def_w, atk_w, ticket, mass)
        _lib.check(_lib.lib.td_sample_weighted(self._h, io, self._stream()))
        return out

    def sample_weighted_boards(self, boards, def_w=None, atk_w=None, ticket=None, mass=False):
        """``sample_weighted`` for the boards named in ``boards`` only (td_sample_weighted_boards),
        the partner of ``step_boards``: every tensor, the weights included, keeps its full-batch
        shape and is indexed by board id, only the named rows are written, and a named board's
        row is the one ``sample_weighted`` gives it under the same ticket.  ``boards`` under
        ``step_boards``' rules; TDError, nothing written: an id out of range or named twice."""
        ids = _board_ids(boards)
        io, out = self._sample_weighted_prepare(def_w, atk_w, ticket, mass)
        _lib.check(_lib.lib.td_sample_weighted_boards(self._h, io, ids.ctypes.data, int(ids.size), self._stream()))
        return out

    def sample_weighted_boards_dev(self, boards, count=None, status=None, def_w=None, atk_w=None, ticket=None,
                                   mass=False):
        """``sample_weighted_boards`` for ids that are on the device
        (td_sample_weighted_boards_dev), the partner of ``step_boards_dev``: nothing is copied
        to the host or waited for.  ``boards``, ``count`` and ``status`` as in
        ``step_boards_dev``; a list the device refuses writes no byte (``list_errors()``).  The
        tensors stay alive until the next call."""
        ids = _dev_ids(boards, self.device, "sample_weighted_boards")
        c = _dev_words(count, 1, self.device, "count")
        st = _dev_words(status, 4, self.device, "status")
        io, out = self._sample_weighted_prepare(def_w, atk_w, ticket, mass)
        _lib.check(_lib.lib.td_sample_weighted_boards_dev(self._h, io, ids.data_ptr(), int(ids.numel()),
                                                          c.data_ptr() if c is not None else None,
                                                          st.data_ptr() if st is not None else None, self._stream()))
        self._keep_sample_list = (ids, c, st)  # alive until the next call's kernels are behind them on the stream
        return out

    def sample_weighted_kernel_name(self):
        """The kernel the three weighted sampling calls launch (td_sample_weighted_kernel_name),
        e.g. 'td_sample_weighted_kernel<10>'."""
        return _lib.lib.td_sample_weighted_kernel_name(self._h).decode()

    # ---------------------------------------------------------------- playouts
    def _playout_prepare(self, steps, ticket, def_idle, atk_idle, first):
        """The engine's playout buffers (allocated on first use) as a td_playout_io for this
        call's ticket, and the tickets the call takes of the engine's sampling counter:
        ``ticket=None`` starts at the counter, which advances by ``steps`` once the call is accepted
        (sub-step j draws at ticket + j); a refused call takes none."""
        B = self.B
        steps = int(steps)
        buf = getattr(self, "_playout_buf", None)
        if buf is None:
            z = lambda dt: torch.zeros(B, dtype=dt, device=self.device)  # noqa: E731
            buf = self._playout_buf = {
                "reward": z(torch.float64), "done": z(torch.uint8), "steps_run": z(torch.int32), "win": z(torch.int8),
                "allow_next": z(torch.uint8), "cooldowns": z(torch.uint8), "ep_return": z(torch.float64),
                "ep_len": z(torch.int32), "first_def": None, "first_atk": None}
        if first:
            if self.mode != "atk" and buf["first_def"] is None:
                buf["first_def"] = torch.full((B,), 6 * self.L * self.L, dtype=torch.int64, device=self.device)
            if self.mode != "def" and buf["first_atk"] is None:
                buf["first_atk"] = torch.full((B, 3, 8), 4, dtype=torch.int64, device=self.device)
        advance = 0  # the counter moves once the library has accepted the call (_playout_done)
        if ticket is None:
            ticket, advance = self._sample_ticket, steps
        io = _lib.TdPlayoutIO(steps=steps, seed=self.sample_seed, ticket=int(ticket) & sampling.M64,
                              def_idle=sampling.idle_units(def_idle), atk_idle=sampling.idle_units(atk_idle))
        out = dict(buf)
        if not first:
            out["first_def"] = out["first_atk"] = None
        for name, t in out.items():
            setattr(io, name, t.data_ptr() if t is not None else None)
        return io, out, advance

    def _playout_done(self, rc, advance):
        """A playout call's return code checked; only an accepted call takes its tickets."""
        _lib.check(rc)
        self._sample_ticket = (self._sample_ticket + advance) & sampling.M64

    def playout(self, steps, boards=None, ticket=None, def_idle=0.0, atk_idle=0.0, first=False):
        """Random playouts on the device (td_playout, td_playout_boards): every board -- or the
        boards named in ``boards``, under ``step_boards``' rules -- is played on for up to
        ``steps`` board steps under the uniform random legal policy, in one kernel and with no
        observation written.  Sub-step j is ``sample_actions_boards`` at ticket + j followed by
        ``step_boards`` (gym_TD.sampling.reference_playout states it on the CPU); a board stops
        after the sub-step that ends its episode, and with auto-reset starts its next one there.

        Returns a dict of the engine's own device tensors, full-batch and indexed by board id
        (allocated on first use, only the played rows overwritten by the next call):
        ``"reward"`` float64 (the sub-steps' rewards added left to right), ``"done"`` uint8,
        ``"steps_run"`` int32, ``"win"``, ``"allow_next"``, ``"cooldowns"``, ``"ep_return"``,
        ``"ep_len"`` as the last executed sub-step would have written them, and with ``first``
        ``"first_def"`` int64 (B,) / ``"first_atk"`` int64 (B, 3, 8): the actions of sub-step 0
        (None without ``first`` and for a side the mode lacks).
        ``ticket=None`` takes the engine's sampling counter and advances it by ``steps`` (a refused
        call takes no ticket).
        ``self.obs`` is not written: the next step writes every byte of it.  One kernel on
        torch's current stream, which must be the stream of step(); nothing is synchronised.
        TDError, nothing changed: ``steps`` outside 1 .. 4096, multi-action, random_agent=False,
        an id out of range or named twice."""
        io, out, advance = self._playout_prepare(steps, ticket, def_idle, atk_idle, first)
        if boards is None:
            self._changed()
            self._playout_done(_lib.lib.td_playout(self._h, io, self._stream()), advance)
        else:
            ids = _board_ids(boards)
            self._changed(("host", ids.copy()))
            self._playout_done(_lib.lib.td_playout_boards(self._h, io, ids.ctypes.data, int(ids.size), self._stream()),
                               advance)
        return out

    def playout_boards_dev(self, boards, steps, count=None, status=None, ticket=None, def_idle=0.0, atk_idle=0.0,
                           first=False):
        """``playout`` for ids that are on the device (td_playout_boards_dev): nothing is copied to
        the host or waited for.  ``boards``, ``count`` and ``status`` as in ``step_boards_dev``; a
        list the device refuses changes no byte (``list_errors()``).  The tensors stay alive
        until the next call."""
        ids = _dev_ids(boards, self.device, "playout")
        c = _dev_words(count, 1, self.device, "count")
        st = _dev_words(status, 4, self.device, "status")
        io, out, advance = self._playout_prepare(steps, ticket, def_idle, atk_idle, first)
        self._changed(("dev", ids, c))
        self._playout_done(_lib.lib.td_playout_boards_dev(self._h, io, ids.data_ptr(), int(ids.numel()),
                                                          c.data_ptr() if c is not None else None,
                                                          st.data_ptr() if st is not None else None, self._stream()),
                           advance)
        self._keep_playout_list = (ids, c, st)  # alive until the next call's kernels are behind them on the stream
        return out

    def playout_kernel_name(self):
        """The kernel the three playout calls launch (td_playout_kernel_name), e.g.
        'td_playout_kernel<10, 0>'."""
        return _lib.lib.td_playout_kernel_name(self._h).decode()

    # ---------------------------------------------------------------- probes
    def _probe_prepare(self, steps, reps, ticket, def_idle, atk_idle, first):
        """The engine's probe buffers -- (B, reps), allocated on first use and again when ``reps``
        grows -- as a td_probe_io for this call's ticket, and the tickets the call takes of the
        engine's sampling counter: ``ticket=None`` starts at the counter, which advances by
        ``steps * reps`` once the call is accepted; a refused call takes none."""
        B = self.B
        steps, reps = int(steps), int(reps)
        width = min(max(reps, 1), _lib.MAX_PROBE_REPS)  # (a refused reps still gets buffers; the call writes none)
        buf = getattr(self, "_probe_buf", None)
        if buf is None or buf["width"] < width:
            z = lambda dt: torch.zeros(B * width, dtype=dt, device=self.device)  # noqa: E731
            buf = self._probe_buf = {"width": width, "reward": z(torch.float64), "done": z(torch.uint8),
                                     "steps_run": z(torch.int32), "win": z(torch.int8), "first_def": None,
                                     "first_atk": None}
        if first:
            if self.mode != "atk" and buf["first_def"] is None:
                buf["first_def"] = torch.full((B * buf["width"],), 6 * self.L * self.L, dtype=torch.int64,
                                              device=self.device)
            if self.mode != "def" and buf["first_atk"] is None:
                buf["first_atk"] = torch.full((B * buf["width"], 3, 8), 4, dtype=torch.int64, device=self.device)
        advance = 0  # the counter moves once the library has accepted the call (_playout_done)
        if ticket is None:
            ticket, advance = self._sample_ticket, steps * reps
        io = _lib.TdProbeIO(steps=steps, reps=reps, seed=self.sample_seed, ticket=int(ticket) & sampling.M64,
                            def_idle=sampling.idle_units(def_idle), atk_idle=sampling.idle_units(atk_idle))
        out = {}
        for name in ("reward", "done", "steps_run", "win", "first_def", "first_atk"):
            t = buf[name] if first or not name.startswith("first") else None
            if t is not None:  # the first B * reps rows of the flat buffer, as [B][reps]
                t = t[:B * width].view((B, width) + tuple(t.shape[1:]))
            out[name] = t
            setattr(io, name, t.data_ptr() if t is not None else None)
        return io, out, advance

    def probe(self, steps, reps, boards=None, ticket=None, def_idle=0.0, atk_idle=0.0, first=False):
        """``reps`` independent random playouts per board, the boards left untouched (td_probe,
        td_probe_boards): every board -- or the boards named in ``boards``, under
        ``step_boards``' rules -- is only read.  Replica r of board b is what
        ``playout(steps, [b], ticket + r * steps)`` would return on the board's present state
        (``gym_TD.sampling.reference_probe`` states it on the CPU); every replica starts from the
        same position of the board's opponent stream, so replicas differ through the sampled side
        only.  A replica stops after the sub-step that ends its episode; nothing is reset.

        Returns a dict of the engine's own (B, reps) device tensors, indexed by board id, then
        replica (allocated on first use, again when ``reps`` grows; only the named boards' rows are
        overwritten by the next call): ``"reward"`` float64, ``"done"`` uint8, ``"steps_run"``
        int32, ``"win"`` int8, and with ``first`` ``"first_def"`` int64 (B, reps) / ``"first_atk"``
        int64 (B, reps, 3, 8) (None without ``first`` and for a side the mode lacks).
        ``ticket=None`` takes the engine's sampling counter and advances it by ``steps * reps`` (a
        refused call takes none).  No board, stream, flag, episode record, staged layout or
        observation byte changes, and a retained observation stays known: the next ``step()``
        skips as if no probe had run.  One kernel on torch's current stream, which must be the
        stream of step(); nothing is synchronised.
        TDError, nothing changed: ``steps`` outside 1 .. 4096, ``reps`` outside 1 .. 256,
        multi-action, random_agent=False, an id out of range or named twice."""
        io, out, advance = self._probe_prepare(steps, reps, ticket, def_idle, atk_idle, first)
        if boards is None:
            self._playout_done(_lib.lib.td_probe(self._h, io, self._stream()), advance)
        else:
            ids = _board_ids(boards)
            self._playout_done(_lib.lib.td_probe_boards(self._h, io, ids.ctypes.data, int(ids.size), self._stream()),
                               advance)
        return out

    def probe_boards_dev(self, boards, steps, reps, count=None, status=None, ticket=None, def_idle=0.0, atk_idle=0.0,
                         first=False):
        """``probe`` for ids that are on the device (td_probe_boards_dev): nothing is copied to the
        host or waited for.  ``boards``, ``count`` and ``status`` as in ``step_boards_dev``; a list
        the device refuses writes no byte (``list_errors()``).  The tensors stay alive until the
        next call."""
        ids = _dev_ids(boards, self.device, "probe")
        c = _dev_words(count, 1, self.device, "count")
        st = _dev_words(status, 4, self.device, "status")
        io, out, advance = self._probe_prepare(steps, reps, ticket, def_idle, atk_idle, first)
        self._playout_done(_lib.lib.td_probe_boards_dev(self._h, io, ids.data_ptr(), int(ids.numel()),
                                                        c.data_ptr() if c is not None else None,
                                                        st.data_ptr() if st is not None else None, self._stream()),
                           advance)
        self._keep_probe_list = (ids, c, st)  # alive until the next call's kernels are behind them on the stream
        return out

    def probe_kernel_name(self):
        """The kernel the three probe calls launch (td_probe_kernel_name), e.g.
        'td_probe_kernel<10, 0>'."""
        return _lib.lib.td_probe_kernel_name(self._h).decode()

    def _changed(self, rows=None):
        """Called in front of every call that can change a board or the config: the state
        serial advances.  rows: the boards the call can change, ``("host", int32 array)`` or
        ``("dev", ids, count)``; None = any board, or the config."""
        self._mask_pending = (self._state_serial, rows) if rows is not None else None
        self._state_serial += 1

    def refresh_action_mask(self, code=False):
        """``action_mask(code)`` -- the same tensors with the same bytes -- at the cost of the
        rows that changed, where the engine knows which: the mask buffers were written whole
        for the state just before the engine's most recent state-changing call, and that call
        was a list step or a board copy.  Then only its boards (the copy's destinations) are
        computed again, by ``action_mask_boards`` or ``action_mask_boards_dev`` on the call's
        own list.  In every other case (the first call, a ``step()``, a reset, a config change, a
        state import, the opponent, or two changes since the last mask) this is ``action_mask``.
        A device list must still hold what the call read."""
        p = self._mask_pending
        keys = ("mask", "code") if code and self.mode != "atk" else ("mask",)
        if p is None or p[0] != self._state_serial - 1 or any(self._mask_at.get(k) != p[0] for k in keys):
            return self.action_mask(code)
        rows = p[1]
        if rows[0] == "host":
            out = self.action_mask_boards(rows[1], code=code)
        else:
            out = self.action_mask_boards_dev(rows[1], count=rows[2], code=code)
        self._mask_pending = None
        for k in keys:
            self._mask_at[k] = self._state_serial
        return out

    # ----------------------------------------------------------------- state
    def state_bytes(self, count):
        return _lib.lib.td_state_bytes(self._h, count)

    def export_state(self, b0=0, count=None):
        """Raw SoA state of boards [b0, b0+count) as numpy arrays (td_export_state).  The
        numpy layout stream is not included: get_np_state / set_np_state carry it (with
        random_agent=False it is the built-in opponent's stream too)."""
        count = self.B - b0 if count is None else count
        buf = np.zeros(self.state_bytes(count), dtype=np.uint8)
        torch.cuda.synchronize(self.device)
        _lib.check(_lib.lib.td_export_state(self._h, b0, count, buf.ctypes.data))
        return _decode_state(buf, count, self.L)

    def import_state(self, st, b0=0):
        count = len(st["hdr"])
        buf = _encode_state(st, count, self.L)
        torch.cuda.synchronize(self.device)
        self._changed()
        _lib.check(_lib.lib.td_import_state(self._h, b0, count, buf.ctypes.data))

    def episode_stats(self, clear=False):
        """Device f64 [2]: episodes finished since the last clear and the sum of their returns."""
        out = torch.empty(2, dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib.td_episode_stats(self._h, _lib.ctypes.c_void_p(out.data_ptr()), int(bool(clear)),
                                             self._stream()))
        return out

    def episode_records(self):
        """Each board's last finished episode (td_episode_records): (return f64 [B],
        length int32 [B], win int32 [B], -1 before the board's first finished episode),
        device tensors -- the per-board payload gathered across ranks."""
        raw = torch.empty((self.B, 16), dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib.td_episode_records(self._h, _lib.ctypes.c_void_p(raw.data_ptr()), self._stream()))
        ints = raw[:, 8:].contiguous().view(torch.int32)
        return raw[:, :8].contiguous().view(torch.float64).reshape(self.B), ints[:, 0], ints[:, 1]

    def opponent(self, side, level, mask=None):
        """Run the built-in opponent on its own (TDGymBasic.py:81-292): side 'enemy'
        (random_enemy_lv<level>) or 'tower' (random_tower_lv<level>), boards in mask."""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint8).reshape(self.B))
        self._changed()
        _lib.check(_lib.lib.td_opponent(self._h, {"enemy": 0, "tower": 1}[side], int(level),
                                        _lib.ptr(m, _lib.ctypes.c_uint8) if m is not None else None, self._stream()))

    def set_step_kernel(self, kind):
        """Select the step kernel: 'auto', 'large', 'small' or 'small2' (td_set_step_kernel)."""
        if kind not in _lib.STEP_KERNELS:
            raise ValueError("step kernel must be one of %s" % sorted(_lib.STEP_KERNELS))
        _lib.check(_lib.lib.td_set_step_kernel(self._h, _lib.STEP_KERNELS[kind]))

    def set_retained_step_kernel(self, kind):
        """The step kernel of skipping launches only -- steps into the retained observation that
        leave clean windows unwritten: 'auto' (the rule), 'large', 'small' or 'small2'
        (td_set_retained_step_kernel, a measurement hook).  set_step_kernel overrides it."""
        if kind not in _lib.STEP_KERNELS:
            raise ValueError("step kernel must be one of %s" % sorted(_lib.STEP_KERNELS))
        _lib.check(_lib.lib.td_set_retained_step_kernel(self._h, _lib.STEP_KERNELS[kind]))

    def set_frame_skip(self, k):
        """Board steps per step() from the next step on (td_set_frame_skip): 1 .. 16.  No
        board state changes; refused (TDError) with k > 1 on a multi-action or
        random_agent=False engine."""
        k = _check_frame_skip(k)
        _lib.check(_lib.lib.td_set_frame_skip(self._h, k))
        self.frame_skip = k

    def set_obs_dtype(self, obs_dtype, obs=None):
        """Switch the observation's element between steps (td_set_obs_format): ``obs`` is
        the new buffer (B, 45, L, L) of that dtype, a fresh one if None.  No board state
        changes; the next step or reset writes the observation in the new form."""
        if obs_dtype not in OBS_FORMATS:
            raise ValueError("obs_dtype must be torch.float32 or torch.float16, not %r" % (obs_dtype,))
        shape = (self.B, _lib.NCH, self.L, self.L)
        own = obs is None
        if obs is None:
            obs = torch.zeros(shape, dtype=obs_dtype).pin_memory() if self.host_io else \
                device_zeros(shape, obs_dtype, self.device)
        if obs.dtype != obs_dtype or tuple(obs.shape) != shape or not obs.is_contiguous():
            raise ValueError("obs must be a contiguous %r tensor of shape %r" % (obs_dtype, shape))
        _lib.check(_lib.lib.td_set_obs_format(self._h, OBS_FORMATS[obs_dtype]))
        self.obs_dtype, self.obs = obs_dtype, obs
        self._io.obs = obs.data_ptr()
        self._arm_retain(own)
        if self.host_io:
            self.np.obs = obs.numpy()

    @property
    def step_kernel(self):
        """The step kernel of a td_step that writes every window: 'large', 'small' or 'small2'."""
        k = _lib.check(_lib.lib.td_step_kernel(self._h))
        return {v: n for n, v in _lib.STEP_KERNELS.items()}[k]

    @property
    def retained_step_kernel(self):
        """The step kernel of a skipping launch (a step into the retained observation):
        'large', 'small' or 'small2' (td_retained_step_kernel)."""
        k = _lib.check(_lib.lib.td_retained_step_kernel(self._h))
        return {v: n for n, v in _lib.STEP_KERNELS.items()}[k]

    @property
    def step_kernel_name(self):
        """The kernel of the most recent step (before the first: of a step that writes every
        window) as rocprofv3 reports it, e.g. 'td_step_kernel_small<10, 0, false>'."""
        return _lib.lib.td_step_kernel_name(self._h).decode()

    def set_store_policy(self, xcd_map=1, edge_wt=2):
        """Board map and shared-line store policy of the step kernels (td_set_store_policy):
        xcd_map 1 = XCD-contiguous boards, 0 = block i steps board i; edge_wt 2 = the lines a
        board shares with its neighbours as plain write-back stores, 1 = write-through.  Every
        policy gives the same bytes; the defaults are the fastest measured."""
        _lib.check(_lib.lib.td_set_store_policy(self._h, int(xcd_map), int(edge_wt)))

    def guard_timeouts(self, clear=False):
        """Ring-guard waits for a board's refill claim that gave up (td_guard_timeouts)."""
        return _lib.check(_lib.lib.td_guard_timeouts(self._h, int(bool(clear))))

    def set_refill_interval(self, steps):
        """Steps between layout-refill launches (auto-reset; 0 = none, rings only drain)."""
        _lib.check(_lib.lib.td_set_refill_interval(self._h, int(steps)))

    def kernel_timing(self, max_launches, every=1):
        """Time the step kernels of every ``every``-th step from now, ``max_launches`` of
        them, from their dispatch timestamps (events bound to the launch itself); read
        them with kernel_times()."""
        _lib.check(_lib.lib.td_kernel_timing(self._h, int(max_launches), int(every)))

    def kernel_times(self):
        """Durations (microseconds, numpy float32) of the step kernels timed since kernel_timing()."""
        cap = 1 << 20
        n = _lib.check(_lib.lib.td_kernel_times(self._h, None, 0))
        out = np.zeros(max(n, 1), dtype=np.float32)
        n = _lib.check(_lib.lib.td_kernel_times(self._h, _lib.ptr(out, _lib.ctypes.c_float), min(n, cap)))
        return out[:n]

    def flags(self):
        f = np.zeros(self.B, dtype=np.int32)
        _lib.check(_lib.lib.td_get_flags(self._h, _lib.ptr(f, _lib.ctypes.c_int32)))
        return f

    def board_state(self, b, st=None):
        """Canonical state of board b (same record as the reference's board attributes)."""
        if st is None:
            st = self.export_state(b, 1)
            i = 0
        else:
            i = b
        h = st["hdr"][i]
        n, nt, L = int(h["n_en"]), int(h["n_tw"]), self.L
        inf = st["en_inf"][i][:n]
        ens = [(int((u >> 12) & 3), int((u >> 14) & 1), int(u & 0xFFF) // L, int(u & 0xFFF) % L, int((u >> 16) & 0xFF),
                float(st["en_lp"][i][k]), float(st["en_mg"][i][k])) for k, u in enumerate(inf)]
        tinf = st["tw_inf"][i][:nt]
        tws = [(int((u >> 12) & 3), int((u >> 14) & 1), int(u & 0xFFF) // L, int(u & 0xFFF) % L,
                float(st["tw_cd"][i][k])) for k, u in enumerate(tinf)]
        return {"steps": int(h["steps"]), "base_LP": int(h["base_LP"]), "cost_def": float(h["cost_def"]),
                "cost_atk": float(h["cost_atk"]), "attacker_cd": int(h["atk_cd"]), "defender_cd": int(h["def_cd"]),
                "enemies": ens, "towers": tws, "map6": (st["cells"][i] >> 24).astype(np.int64).tolist(),
                "num_roads": int(h["num_roads"]), "flags": int(h["flags"])}

    def map_planes(self, b, st=None):
        """TDBoard.map planes 0-6 of board b (int32 (7, L, L)), start list, end."""
        if st is None:
            st = self.export_state(b, 1)
            b = 0
        cw = st["cells"][b].astype(np.int64)
        L = self.L
        m = np.zeros((7, L, L), dtype=np.int32)
        for p in range(4):
            m[p] = ((cw >> p) & 1).reshape(L, L)
        m[4] = ((cw >> 16) & 0xFF).reshape(L, L)
        m[5] = ((cw >> 8) & 3).reshape(L, L)
        m[6] = (cw >> 24).reshape(L, L)
        h = st["hdr"][b]
        nr = int(h["num_roads"])
        start = [[int(c) // L, int(c) % L] for c in h["start_cell"][:nr]]
        end = [int(h["end_cell"]) // L, int(h["end_cell"]) % L]
        return m, start, end


def _check_frame_skip(k):
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= _lib.MAX_FRAME_SKIP:
        raise ValueError("frame_skip must be an int in [1, %d], not %r" % (_lib.MAX_FRAME_SKIP, k))
    return int(k)


def _board_ids(x):
    """Board ids (ints, numpy array, CPU or GPU tensor) -> contiguous int32 host array."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x).reshape(-1)
    if a.dtype == np.int32:  # (the cheap way in: nothing is converted)
        return np.ascontiguousarray(a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("board ids must be integers, not %s" % a.dtype)
    if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) >= 2 ** 31):
        raise ValueError("board id out of range")
    return np.ascontiguousarray(a, dtype=np.int32)


def _dev_ids(x, device, host_method):
    """Board ids on the engine's device -> contiguous int32 device tensor, without a copy to the host."""
    if not isinstance(x, torch.Tensor) or x.device != device:
        raise ValueError("board ids must be an integer tensor on %s; for ids on the host use %s()" % (device, host_method))
    if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
        raise ValueError("board ids must be integers, not %s" % x.dtype)
    x = x.detach().reshape(-1)
    if x.dtype != torch.int32 or not x.is_contiguous():
        x = x.to(torch.int32).contiguous()
    return x


def _dev_words(x, n, device, what):
    """None, or an int32 device tensor of n elements (count, status), taken as it is."""
    if x is None:
        return None
    if not isinstance(x, torch.Tensor) or x.device != device or x.dtype != torch.int32 or x.numel() != n \
            or not x.is_contiguous():
        raise ValueError("%s must be a contiguous int32 tensor of %d element(s) on %s" % (what, n, device))
    return x


def _as_dev(x, dtype, device):
    if isinstance(x, torch.Tensor):
        if x.device != device or x.dtype != dtype or not x.is_contiguous():
            x = x.to(device=device, dtype=dtype).contiguous()
        return x
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(device).contiguous()


def _mt_words(state):
    """random.getstate() / RandomState.get_state() / 625 words -> uint32[625]."""
    if isinstance(state, tuple) and len(state) == 3 and isinstance(state[1], tuple):  # CPython random
        return _u32(list(state[1]))
    if isinstance(state, tuple) and len(state) >= 3 and state[0] == "MT19937":  # numpy RandomState
        return _u32(list(state[1]) + [int(state[2])])
    w = _u32(state)
    if w.shape != (_lib.MT_WORDS,):
        raise ValueError("expected 625 words")
    return w


def _layout(count, L):
    return [("hdr", HDR_DTYPE, ()), ("en_lp", np.float64, (_lib.ECAP,)), ("en_mg", np.float64, (_lib.ECAP,)),
            ("en_inf", np.uint32, (_lib.ECAP,)), ("tw_cd", np.float64, (_lib.TCAP,)),
            ("tw_inf", np.uint32, (_lib.TCAP,)), ("cells", np.uint32, (L * L,)),
            ("opp_mt", np.uint32, (_lib.OPP_WORDS,))]


def _decode_state(buf, count, L):
    out, off = {}, 0
    for name, dt, shape in _layout(count, L):
        dt = np.dtype(dt)
        n = count * int(np.prod(shape, dtype=np.int64)) if shape else count
        a = np.frombuffer(buf, dtype=dt, count=n, offset=off)
        out[name] = a.reshape((count,) + shape) if shape else a
        off += n * dt.itemsize
    return out


def _encode_state(st, count, L):
    parts = []
    for name, dt, shape in _layout(count, L):
        parts.append(np.ascontiguousarray(st[name], dtype=dt).tobytes())
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


def layout_planes(rec, L):
    """Layout record (td_layout.h) -> (map planes int32 (7, L, L), start list, end, num_roads)."""
    rec = np.asarray(rec, dtype=np.uint32)
    cw = rec[8:8 + L * L].astype(np.int64)
    m = np.zeros((7, L, L), dtype=np.int32)
    for p in range(4):
        m[p] = ((cw >> p) & 1).reshape(L, L)
    m[4] = ((cw >> 16) & 0xFF).reshape(L, L)
    m[5] = ((cw >> 8) & 3).reshape(L, L)
    m[6] = (cw >> 24).reshape(L, L)
    nr = int(rec[1])
    start = [[int(c) // L, int(c) % L] for c in rec[4:4 + nr]]
    end = [int(rec[2]) // L, int(rec[2]) % L]
    return m, start, end, nr


def generate_layout(np_state, L, max_attempts=20000):
    """TDGymBasic.reset's draws (num_roads + create_road_v2) on a 625-word numpy
    stream, in place; returns (status, record)."""
    rec = np.zeros(8 + L * L, dtype=np.uint32)
    st = _lib.lib.td_layout_generate(_lib.ptr(np_state, _lib.ctypes.c_uint32), L, max_attempts,
                                     _lib.ptr(rec, _lib.ctypes.c_uint32))
    return st, rec
