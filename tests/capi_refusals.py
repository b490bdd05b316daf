"""What the C ABI refuses, and in which order: one table of bad calls (and the few empty ones it
accepts), each row an entry point, the handle it needs (or none) and its arguments, replayed on a
library and compared with tests/golden/capi_refusals.json -- the return value and the whole
td_last_error() text, byte for byte.

    python tests/capi_refusals.py --record PATH     # writes what the loaded library answers

The golden file was recorded from the library before td_capi.hip's checks were written once each
(select a library with TDSTEP_LIB), the sampler's rows at its end from the library before the
list forms of the masks and the sampler were written once.  Messages that carry a source line (HIP failures) are no
refusals and have no row.

Handles, B = 4 each, the smallest that reach every branch:
    def   L = 10 TD-def, discrete            2p    L = 10 TD-2p, multi-action
    atk   L = 12 TD-atk (the generic map side: no small-batch kernel)
    skip  L = 10 TD-def at frame skip 2      np    L = 10 TD-def, random_agent = 0, auto-reset on
No handle is reset and no row launches a kernel: a refusal returns before anything is enqueued, and
the accepted rows are empty lists and settings that are already in place.  Every device pointer a
row passes is a real allocation of the size a launch would need, its lists hold valid ids.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_refusals.json")
B = 4
HANDLES = {  # name: (L, mode, multi_action)
    "def": (10, 0, 0), "2p": (10, 2, 1), "atk": (12, 1, 0), "skip": (10, 0, 0), "np": (10, 0, 0)}
INT_MIN = -2 ** 31


def _step_rows(fn, tail, dev):
    """The io rows every stepping entry point shares; tail: the arguments after io of a call that
    would be accepted.  dev: the _dev form, whose cap < 0 stands in front of the handle."""
    rows = [
        (fn + " NULL io", fn, None, dict(tail, io="null")),
        (fn + " ABI-2 io", fn, None, dict(tail, io="abi2")),
        (fn + " short io", fn, None, dict(tail, io="size112")),
        (fn + " NULL handle", fn, None, dict(tail, io="ok")),
        (fn + " no obs", fn, "def", dict(tail, io="no_obs")),
        (fn + " no reward", fn, "def", dict(tail, io="no_reward")),
        (fn + " no def_act on TD-def", fn, "def", dict(tail, io="no_def_act")),
        (fn + " no atk_act on TD-atk", fn, "atk", dict(tail, io="no_atk_act")),
        (fn + " no atk_act on TD-2p", fn, "2p", dict(tail, io="no_atk_act")),
        (fn + " no def_act on TD-2p", fn, "2p", dict(tail, io="no_def_act")),
    ]
    if dev:
        rows += [
            (fn + " NULL io, cap < 0", fn, None, dict(tail, io="null", cap=-1)),
            (fn + " ABI-2 io, cap < 0", fn, None, dict(tail, io="abi2", cap=-1)),
            (fn + " short io, cap < 0, a handle", fn, "def", dict(tail, io="size112", cap=-3)),
            (fn + " cap < 0, NULL handle", fn, None, dict(tail, io="ok", cap=-1)),
            (fn + " cap < 0, no obs", fn, "def", dict(tail, io="no_obs", cap=-1)),
        ]
    return rows


def _mask_rows(fn, tail, dev):
    rows = [
        (fn + " NULL io", fn, None, dict(tail, io="null")),
        (fn + " ABI-2 io", fn, None, dict(tail, io="abi2")),
        (fn + " short io", fn, None, dict(tail, io="size24")),
        (fn + " NULL handle", fn, None, dict(tail, io="ok")),
        (fn + " no output", fn, "def", dict(tail, io="none")),
        (fn + " no output, TD-atk", fn, "atk", dict(tail, io="none")),
        (fn + " no output, a pitch, multi-action", fn, "2p", dict(tail, io="none", pitch=1)),
        (fn + " def_mask on TD-atk", fn, "atk", dict(tail, io="def_mask")),
        (fn + " def_code on TD-atk", fn, "atk", dict(tail, io="def_code")),
        (fn + " atk_mask on TD-def", fn, "def", dict(tail, io="atk_mask")),
        (fn + " both sides on TD-def", fn, "def", dict(tail, io="both")),
        (fn + " both sides on TD-atk", fn, "atk", dict(tail, io="both")),
        (fn + " pitch on multi-action", fn, "2p", dict(tail, io="def_mask", pitch=1024)),
        (fn + " pitch too small on multi-action", fn, "2p", dict(tail, io="def_mask", pitch=1)),
        (fn + " pitch one short", fn, "def", dict(tail, io="def_mask", pitch=600)),
        (fn + " pitch too large", fn, "def", dict(tail, io="def_code", pitch=2 ** 40)),
        (fn + " pitch with atk_mask on TD-def", fn, "def", dict(tail, io="atk_mask", pitch=1)),
    ]
    if dev:
        rows += [
            (fn + " NULL io, cap < 0", fn, None, dict(tail, io="null", cap=-1)),
            (fn + " ABI-2 io, cap < 0", fn, None, dict(tail, io="abi2", cap=-1)),
            (fn + " short io, cap < 0, a handle", fn, "def", dict(tail, io="size24", cap=-3)),
            (fn + " cap < 0, NULL handle", fn, None, dict(tail, io="ok", cap=-1)),
            (fn + " cap < 0, no output", fn, "def", dict(tail, io="none", cap=-1)),
        ]
    return rows


def _sample_rows(fn, tail, dev):
    """The io rows of the sampling entry points, as _mask_rows; an io kind names the outputs it has
    (SAMPLE_OUTS)."""
    rows = [
        (fn + " NULL io", fn, None, dict(tail, io="null")),
        (fn + " ABI-2 io", fn, None, dict(tail, io="abi2")),
        (fn + " short io", fn, None, dict(tail, io="size56")),
        (fn + " NULL handle", fn, None, dict(tail, io="ok")),
        (fn + " no action output", fn, "def", dict(tail, io="none")),
        (fn + " no action output, TD-atk", fn, "atk", dict(tail, io="none")),
        (fn + " no action output, both counts", fn, "2p", dict(tail, io="counts")),
        (fn + " def_act on TD-atk", fn, "atk", dict(tail, io="def_act")),
        (fn + " def_count on TD-atk", fn, "atk", dict(tail, io="atk_act+def_count")),
        (fn + " atk_act on TD-def", fn, "def", dict(tail, io="atk_act")),
        (fn + " atk_count on TD-def", fn, "def", dict(tail, io="def_act+atk_count")),
        (fn + " both sides on TD-def", fn, "def", dict(tail, io="both")),
        (fn + " both sides on TD-atk", fn, "atk", dict(tail, io="both")),
    ]
    if dev:
        rows += [
            (fn + " NULL io, cap < 0", fn, None, dict(tail, io="null", cap=-1)),
            (fn + " ABI-2 io, cap < 0", fn, None, dict(tail, io="abi2", cap=-1)),
            (fn + " short io, cap < 0, a handle", fn, "def", dict(tail, io="size56", cap=-3)),
            (fn + " cap < 0, NULL handle", fn, None, dict(tail, io="ok", cap=-1)),
            (fn + " cap < 0, no action output", fn, "def", dict(tail, io="none", cap=-1)),
        ]
    return rows


SAMPLE_OUTS = {"ok": ("def_act",), "abi2": ("def_act",), "size56": ("def_act",), "none": (),
               "counts": ("def_count", "atk_count"), "both": ("def_act", "atk_act")}


def _ids_rows(fn, io):
    """A host list's refusals (td_ids_check.h) behind an io that passes."""
    return [
        (fn + " n = -1", fn, "def", dict(io=io, boards=[0], n=-1)),
        (fn + " n = INT_MIN, NULL ids", fn, "def", dict(io=io, boards=None, n=INT_MIN)),
        (fn + " n = B + 1", fn, "def", dict(io=io, boards=[0, 1, 2, 3, 0], n=B + 1)),
        (fn + " n = 0, NULL ids", fn, "def", dict(io=io, boards=None, n=0)),
        (fn + " n = 0, ids", fn, "def", dict(io=io, boards=[9], n=0)),
        (fn + " n = 1, NULL ids", fn, "def", dict(io=io, boards=None, n=1)),
        (fn + " id -1", fn, "def", dict(io=io, boards=[-1], n=1)),
        (fn + " id B at the back", fn, "def", dict(io=io, boards=[0, 1, B], n=3)),
        (fn + " twice", fn, "def", dict(io=io, boards=[2, 1, 2], n=3)),
        (fn + " range before twice", fn, "def", dict(io=io, boards=[0, 9, 0], n=3)),
        (fn + " twice before range", fn, "def", dict(io=io, boards=[0, 0, 9], n=3)),
        (fn + " twice on TD-2p", fn, "2p", dict(io=io, boards=[3, 3], n=2)),
    ]


def _cap_rows(fn, io, lists):
    """A device list's host-side refusals; lists: the list arguments of the call."""
    ok = {k: "ok" for k in lists}
    rows = [
        (fn + " cap = -1", fn, "def", dict(ok, io=io, cap=-1)),
        (fn + " cap = INT_MIN, NULL lists", fn, "def", dict({k: None for k in lists}, io=io, cap=INT_MIN)),
        (fn + " cap = B + 1", fn, "def", dict(ok, io=io, cap=B + 1)),
        (fn + " cap = B + 1, NULL lists", fn, "atk", dict({k: None for k in lists}, io=io, cap=B + 1)),
        (fn + " cap = 0, NULL lists", fn, "def", dict({k: None for k in lists}, io=io, cap=0)),
        (fn + " cap = 0, NULL count and status", fn, "2p", dict(ok, io=io, cap=0, count=None, status=None)),
        (fn + " cap = 1, NULL lists", fn, "def", dict({k: None for k in lists}, io=io, cap=1)),
    ]
    for k in lists:
        rows.append((fn + " cap = B, NULL " + k, fn, "def", dict(ok, io=io, cap=B, **{k: None})))
    return rows


def _kind_rows(fn):
    return [
        (fn + " NULL handle", fn, None, dict(kind=2)),
        (fn + " NULL handle, unknown kind", fn, None, dict(kind=9)),
        (fn + " kind -1", fn, "def", dict(kind=-1)),
        (fn + " kind 4", fn, "def", dict(kind=4)),
        (fn + " small on L = 12", fn, "atk", dict(kind=2)),
        (fn + " small2 on L = 12", fn, "atk", dict(kind=3)),
        (fn + " unknown kind on L = 12", fn, "atk", dict(kind=4)),
        (fn + " kind INT_MIN on L = 12", fn, "atk", dict(kind=INT_MIN)),
        (fn + " auto on L = 12", fn, "atk", dict(kind=0)),
        (fn + " auto on L = 10", fn, "def", dict(kind=0)),
    ]


def table():
    """[(id, entry point, handle name or None, arguments)], in replay order."""
    t = []
    # ---- the stepping calls
    t += _step_rows("td_step", {}, False)
    t += _step_rows("td_step_boards", dict(boards=[0], n=1), False)
    t += _ids_rows("td_step_boards", "ok")
    fn = "td_step_boards"
    t += [
        (fn + " frame skip", fn, "skip", dict(io="ok", boards=[0], n=1)),
        (fn + " frame skip, n = 0", fn, "skip", dict(io="ok", boards=None, n=0)),
        (fn + " frame skip, n > B", fn, "skip", dict(io="ok", boards=[0], n=B + 1)),
        (fn + " frame skip, twice", fn, "skip", dict(io="ok", boards=[1, 1], n=2)),
        (fn + " frame skip, no obs", fn, "skip", dict(io="no_obs", boards=[0], n=1)),
        (fn + " random_agent = 0", fn, "np", dict(io="ok", boards=[0], n=1)),
        (fn + " random_agent = 0, n = 0", fn, "np", dict(io="ok", boards=None, n=0)),
        (fn + " random_agent = 0, id out of range", fn, "np", dict(io="ok", boards=[B], n=1)),
        (fn + " random_agent = 0, no def_act", fn, "np", dict(io="no_def_act", boards=[0], n=1)),
        (fn + " no obs, twice", fn, "def", dict(io="no_obs", boards=[1, 1], n=2)),
    ]
    fn = "td_step_boards_dev"
    t += _step_rows(fn, dict(boards="ok", cap=1), True)
    t += _cap_rows(fn, "ok", ["boards"])
    t += [
        (fn + " frame skip", fn, "skip", dict(io="ok", boards="ok", cap=1)),
        (fn + " frame skip, cap = 0", fn, "skip", dict(io="ok", boards="ok", cap=0)),
        (fn + " frame skip, cap > B", fn, "skip", dict(io="ok", boards="ok", cap=B + 1)),
        (fn + " frame skip, cap < 0", fn, "skip", dict(io="ok", boards="ok", cap=-1)),
        (fn + " frame skip, NULL list", fn, "skip", dict(io="ok", boards=None, cap=1)),
        (fn + " random_agent = 0", fn, "np", dict(io="ok", boards="ok", cap=1)),
        (fn + " random_agent = 0, cap = 0", fn, "np", dict(io="ok", boards=None, cap=0)),
        (fn + " random_agent = 0, cap > B", fn, "np", dict(io="ok", boards="ok", cap=B + 1)),
        (fn + " random_agent = 0, a list with an id out of range", fn, "np", dict(io="ok", boards="bad", cap=B)),
        (fn + " no obs, cap > B", fn, "def", dict(io="no_obs", boards="ok", cap=B + 1)),
    ]
    # ---- the copies
    fn = "td_copy_boards"
    t += [
        (fn + " NULL handle", fn, None, dict(src=[0], dst=[1], n=1)),
        (fn + " NULL handle, n = -1", fn, None, dict(src=None, dst=None, n=-1)),
        (fn + " n = -1", fn, "def", dict(src=[0], dst=[1], n=-1)),
        (fn + " n = B + 1", fn, "def", dict(src=[0] * 5, dst=[1] * 5, n=B + 1)),
        (fn + " n = 0, NULL ids", fn, "def", dict(src=None, dst=None, n=0)),
        (fn + " n = 0, NULL ids and obs", fn, "2p", dict(src=None, dst=None, n=0, obs=None)),
        (fn + " n = 1, NULL src", fn, "def", dict(src=None, dst=[1], n=1)),
        (fn + " n = 1, NULL dst", fn, "def", dict(src=[0], dst=None, n=1)),
        (fn + " src out of range", fn, "def", dict(src=[0, B], dst=[1, 2], n=2)),
        (fn + " dst -1", fn, "def", dict(src=[0, 0], dst=[1, -1], n=2)),
        (fn + " dst twice", fn, "def", dict(src=[0, 0], dst=[1, 1], n=2)),
        (fn + " source and destination", fn, "def", dict(src=[0, 1], dst=[1, 2], n=2)),
        (fn + " a board onto itself", fn, "atk", dict(src=[3], dst=[3], n=1)),
        (fn + " range before overlap", fn, "def", dict(src=[0, 1, 7], dst=[1, 2, 3], n=3)),
        (fn + " frame skip, dst twice", fn, "skip", dict(src=[0, 0], dst=[1, 1], n=2)),
    ]
    fn = "td_copy_boards_dev"
    t += [
        (fn + " NULL handle", fn, None, dict(src="ok", dst="ok", cap=1)),
        (fn + " cap < 0, NULL handle", fn, None, dict(src="ok", dst="ok", cap=-1)),
        (fn + " cap < 0, NULL everything", fn, None, dict(src=None, dst=None, cap=INT_MIN, count=None, status=None,
                                                             obs=None)),
    ]
    t += _cap_rows(fn, None, ["src", "dst"])
    # ---- the masks
    t += _mask_rows("td_action_mask", {}, False)
    fn = "td_action_mask_boards"
    t += _mask_rows(fn, dict(boards=[0], n=1), False)
    t += _ids_rows(fn, "def_mask")
    t += [
        (fn + " no output, n = -1", fn, "def", dict(io="none", boards=[0], n=-1)),
        (fn + " atk_mask on TD-def, twice", fn, "def", dict(io="atk_mask", boards=[1, 1], n=2)),
        (fn + " pitch one short, id out of range", fn, "def", dict(io="def_mask", pitch=600, boards=[B], n=1)),
        (fn + " frame skip, twice", fn, "skip", dict(io="def_mask", boards=[1, 1], n=2)),
        (fn + " random_agent = 0, n = 0", fn, "np", dict(io="def_code", boards=None, n=0)),
    ]
    fn = "td_action_mask_boards_dev"
    t += _mask_rows(fn, dict(boards="ok", cap=1), True)
    t += _cap_rows(fn, "def_mask", ["boards"])
    t += [
        (fn + " no output, cap > B", fn, "def", dict(io="none", boards="ok", cap=B + 1)),
        (fn + " def_mask on TD-atk, NULL list", fn, "atk", dict(io="def_mask", boards=None, cap=1)),
        (fn + " atk_mask on TD-atk, cap > B", fn, "atk", dict(io="atk_mask", boards="ok", cap=B + 1)),
        (fn + " frame skip, cap = 0", fn, "skip", dict(io="def_mask", boards=None, cap=0)),
    ]
    # ---- the settings
    t += _kind_rows("td_set_step_kernel")
    t += _kind_rows("td_set_retained_step_kernel")
    fn = "td_set_frame_skip"
    t += [
        (fn + " NULL handle", fn, None, dict(k=2)),
        (fn + " NULL handle, k = 0", fn, None, dict(k=0)),
        (fn + " k = 0", fn, "def", dict(k=0)),
        (fn + " k = -1", fn, "def", dict(k=-1)),
        (fn + " k = 17", fn, "def", dict(k=17)),
        (fn + " k = 2 on multi-action", fn, "2p", dict(k=2)),
        (fn + " k = 17 on multi-action", fn, "2p", dict(k=17)),
        (fn + " k = 1 on multi-action", fn, "2p", dict(k=1)),
        (fn + " k = 2 with random_agent = 0", fn, "np", dict(k=2)),
        (fn + " k = 0 with random_agent = 0", fn, "np", dict(k=0)),
        (fn + " k = 1 with random_agent = 0", fn, "np", dict(k=1)),
        (fn + " k = 2 again", fn, "skip", dict(k=2)),
    ]
    fn = "td_set_obs_format"
    t += [
        (fn + " NULL handle", fn, None, dict(fmt=1)),
        (fn + " NULL handle, unknown format", fn, None, dict(fmt=2)),
        (fn + " format 2", fn, "def", dict(fmt=2)),
        (fn + " format -1", fn, "atk", dict(fmt=-1)),
        (fn + " float32 again", fn, "def", dict(fmt=0)),
    ]
    # ---- the sampler (behind the settings: its rows were recorded later, at the golden file's end)
    t += _sample_rows("td_sample_actions", {}, False)
    fn = "td_sample_actions_boards"
    t += _sample_rows(fn, dict(boards=[0], n=1), False)
    t += _ids_rows(fn, "def_act")
    t += [
        (fn + " no action output, n = -1", fn, "def", dict(io="none", boards=[0], n=-1)),
        (fn + " atk_act on TD-def, twice", fn, "def", dict(io="atk_act", boards=[1, 1], n=2)),
        (fn + " frame skip, twice", fn, "skip", dict(io="def_act", boards=[1, 1], n=2)),
        (fn + " random_agent = 0, n = 0", fn, "np", dict(io="def_act+def_count", boards=None, n=0)),
    ]
    fn = "td_sample_actions_boards_dev"
    t += _sample_rows(fn, dict(boards="ok", cap=1), True)
    t += _cap_rows(fn, "def_act", ["boards"])
    t += [
        (fn + " no action output, cap > B", fn, "def", dict(io="none", boards="ok", cap=B + 1)),
        (fn + " def_act on TD-atk, NULL list", fn, "atk", dict(io="def_act", boards=None, cap=1)),
        (fn + " atk_act on TD-atk, cap > B", fn, "atk", dict(io="atk_act", boards="ok", cap=B + 1)),
        (fn + " frame skip, cap = 0", fn, "skip", dict(io="def_act", boards=None, cap=0)),
    ]
    ids = [r[0] for r in t]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return t


class Fixtures:
    """The handles and the device memory the rows of one kind of run point to.  gpu = False: no
    handle, and any non-NULL address for a device pointer -- a call without a handle reads no
    argument but its io's two header words."""

    def __init__(self, lib_mod, gpu):
        self._lib = lib_mod
        self.lib = lib_mod.lib
        self.gpu = gpu
        self.h = {}
        self.keep = []
        self.dev = {}
        if not gpu:
            return
        import torch
        cfg = lib_mod.TdConfig()
        self.lib.td_config_default(ctypes.byref(cfg))
        for name, (L, mode, multi) in HANDLES.items():
            h = self.lib.td_create(ctypes.byref(cfg), L, B, mode, multi, 1, 0)
            assert h, self.lib.td_last_error()
            self.h[name] = h
        assert self.lib.td_set_frame_skip(self.h["skip"], 2) == 0, self.lib.td_last_error()
        assert self.lib.td_set_random_agent(self.h["np"], 0) == 0, self.lib.td_last_error()
        # one set of buffers, sized for the largest handle (L = 12; multi-action actions [B][6][L][L])
        cells = 12 * 12
        d = dict(device="cuda:0")
        self.dev = {
            "obs": torch.zeros(B * lib_mod.NCH * cells, dtype=torch.float32, **d),
            "reward": torch.zeros(B, dtype=torch.float32, **d),
            "done": torch.zeros(B, dtype=torch.uint8, **d),
            "def_act": torch.zeros(B * 6 * cells, dtype=torch.int64, **d),
            "atk_act": torch.zeros(B * 3 * 4, dtype=torch.int64, **d),
            "def_mask": torch.zeros(B * 1024, dtype=torch.uint8, **d),
            "def_code": torch.zeros(B * 1024, dtype=torch.uint8, **d),
            "atk_mask": torch.zeros(B * 64, dtype=torch.uint8, **d),
            "sample_atk_act": torch.zeros(B * 3 * 8, dtype=torch.int64, **d),
            "def_count": torch.zeros(B, dtype=torch.int32, **d),
            "atk_count": torch.zeros(B, dtype=torch.int32, **d),
            "ok": torch.arange(B, dtype=torch.int32, **d),
            "ok2": torch.arange(B, dtype=torch.int32, **d),
            "bad": torch.tensor([0, 1, B, 2], dtype=torch.int32, **d),
            "count": torch.tensor([1], dtype=torch.int32, **d),
            "status": torch.zeros(4, dtype=torch.int32, **d),
        }
        torch.cuda.synchronize()

    def close(self):
        for h in self.h.values():
            self.lib.td_destroy(h)
        self.h = {}

    def ptr(self, name):
        if name is None:
            return None
        return self.dev[name].data_ptr() if self.gpu else 0x1000

    def step_io(self, kind):
        if kind == "null":
            return None
        io = self._lib.TdStepIO(**{k: self.ptr(k) for k in ("def_act", "atk_act", "obs", "reward", "done")})
        if kind == "abi2":
            io.abi = 2
        elif kind == "size112":
            io.size = 112
        elif kind.startswith("no_"):
            setattr(io, kind[3:], None)
        else:
            assert kind == "ok", kind
        return io

    def mask_io(self, kind, pitch):
        if kind == "null":
            return None
        outs = {"ok": ("def_mask",), "abi2": ("def_mask",), "size24": ("def_mask",), "none": (), "both":
                ("def_mask", "atk_mask")}.get(kind, (kind,))
        io = self._lib.TdMaskIO(def_pitch=pitch, **{k: self.ptr(k) for k in outs})
        if kind == "abi2":
            io.abi = 2
        elif kind == "size24":
            io.size = 24
        return io

    def sample_io(self, kind):
        if kind == "null":
            return None
        outs = SAMPLE_OUTS.get(kind, tuple(kind.split("+")))
        io = self._lib.TdSampleIO(**{k: self.ptr("sample_atk_act" if k == "atk_act" else k) for k in outs})
        if kind == "abi2":
            io.abi = 2
        elif kind == "size56":
            io.size = 56
        return io

    def ids(self, v):
        """A host id array (kept alive to the end of the run), or NULL."""
        if v is None:
            return None
        a = (ctypes.c_int32 * max(len(v), 1))(*v)
        self.keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p)

    def call(self, fn, hname, a):
        """One row: (return value, message or None where the call was accepted)."""
        lib, h = self.lib, self.h.get(hname)
        assert (hname is None) == (h is None), hname
        f = getattr(lib, fn)
        count = self.ptr(a.get("count", "count"))
        status = self.ptr(a.get("status", "status"))
        if fn == "td_step":
            rc = f(h, self.step_io(a["io"]), None)
        elif fn == "td_step_boards":
            rc = f(h, self.step_io(a["io"]), self.ids(a["boards"]), a["n"], None)
        elif fn == "td_step_boards_dev":
            rc = f(h, self.step_io(a["io"]), self.ptr(a["boards"]), a["cap"], count, status, None)
        elif fn == "td_copy_boards":
            rc = f(h, self.ids(a["src"]), self.ids(a["dst"]), a["n"], self.ptr(a.get("obs", "obs")), None)
        elif fn == "td_copy_boards_dev":
            dst = "ok2" if a["dst"] == "ok" else a["dst"]
            rc = f(h, self.ptr(a["src"]), self.ptr(dst), a["cap"], count, self.ptr(a.get("obs", "obs")), status, None)
        elif fn == "td_action_mask":
            rc = f(h, self.mask_io(a["io"], a.get("pitch", 0)), None)
        elif fn == "td_action_mask_boards":
            rc = f(h, self.mask_io(a["io"], a.get("pitch", 0)), self.ids(a["boards"]), a["n"], None)
        elif fn == "td_action_mask_boards_dev":
            rc = f(h, self.mask_io(a["io"], a.get("pitch", 0)), self.ptr(a["boards"]), a["cap"], count, status, None)
        elif fn == "td_sample_actions":
            rc = f(h, self.sample_io(a["io"]), None)
        elif fn == "td_sample_actions_boards":
            rc = f(h, self.sample_io(a["io"]), self.ids(a["boards"]), a["n"], None)
        elif fn == "td_sample_actions_boards_dev":
            rc = f(h, self.sample_io(a["io"]), self.ptr(a["boards"]), a["cap"], count, status, None)
        elif fn in ("td_set_step_kernel", "td_set_retained_step_kernel"):
            rc = f(h, a["kind"])
        elif fn == "td_set_frame_skip":
            rc = f(h, a["k"])
        elif fn == "td_set_obs_format":
            rc = f(h, a["fmt"])
        else:
            raise AssertionError(fn)
        return rc, (lib.td_last_error().decode() if rc < 0 else None)


def replay(lib_mod, gpu):
    """{row id: [return value, message]} of the rows this kind of run can make: all of them with a
    GPU, those that need no handle without."""
    fx = Fixtures(lib_mod, gpu)
    try:
        out = {}
        for rid, fn, hname, args in table():
            if hname is None or gpu:
                out[rid] = list(fx.call(fn, hname, args))
        if gpu:
            import torch
            torch.cuda.synchronize()
        return out
    finally:
        fx.close()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def main(argv):
    if len(argv) != 3 or argv[1] != "--record":
        print(__doc__)
        return 2
    for p in (ROOT, os.path.join(ROOT, "gym-td_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from gym_TD import _lib
    got = replay(_lib, True)
    for rid, (rc, msg) in got.items():
        assert msg is None or ".hip:" not in msg, (rid, msg)  # a HIP failure is no refusal
    with open(argv[2], "w") as f:
        json.dump(got, f, indent=1, sort_keys=False)
        f.write("\n")
    print("capi_refusals: %d rows from %s" % (len(got), _lib.LIB_PATH))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
