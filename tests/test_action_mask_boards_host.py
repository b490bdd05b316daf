"""td_action_mask_boards / td_action_mask_boards_dev / td_action_mask_boards_kernel_name as the
header declares them and the ctypes binding binds them, the unchanged ABI, the refusals that
need no device, and the Python surface's promises -- all without a GPU."""
import ctypes
import re

from gym_TD import _lib

from test_step_boards_host import HEADER, _decl

NAMES = ("td_action_mask_boards", "td_action_mask_boards_dev", "td_action_mask_boards_kernel_name")


def test_header_declares_library_exports_binding_binds():
    src = open(HEADER).read()
    want = {
        "td_action_mask_boards": ("int", ["td_handle*", "const td_mask_io*", "const int32_t*", "int", "void*"]),
        "td_action_mask_boards_dev": ("int", ["td_handle*", "const td_mask_io*", "const int32_t*", "int",
                                              "const int32_t*", "td_list_status*", "void*"]),
        "td_action_mask_boards_kernel_name": ("const char*", ["td_handle*"]),
    }
    for name in NAMES:
        assert _decl(src, name) == want[name], name
        fn = getattr(_lib.lib, name)  # (AttributeError: the library does not export it)
        assert len(fn.argtypes) == len(want[name][1]), name
        assert fn.restype == (ctypes.c_char_p if name.endswith("_name") else ctypes.c_int)
    io = ctypes.POINTER(_lib.TdMaskIO)
    assert list(_lib.lib.td_action_mask_boards.argtypes) == [_lib.c_vp, io, _lib.c_vp, ctypes.c_int, _lib.c_vp]
    assert list(_lib.lib.td_action_mask_boards_dev.argtypes) == [_lib.c_vp, io, _lib.c_vp, ctypes.c_int, _lib.c_vp,
                                                                 _lib.c_vp, _lib.c_vp]
    assert _lib.lib.td_action_mask_boards_kernel_name(None) == b""
    # beside td_action_mask, in the drop-in header
    assert src.index("int td_action_mask(") < src.index("int td_action_mask_boards(") < \
        src.index("int td_action_mask_boards_dev(") < src.index("td_action_mask_boards_kernel_name(")


def test_abi_and_mask_io_unchanged():
    assert re.search(r"#define TD_ABI_VERSION 3\b", open(HEADER).read())
    assert _lib.ABI_VERSION == 3 and _lib.lib.td_abi_version() == 3
    assert ctypes.sizeof(_lib.TdMaskIO) == 40


def test_header_states_the_contract():
    src = open(HEADER).read()
    at = src.index("int td_action_mask_boards(")
    doc = " ".join(src[src.rindex("/*", 0, at):at].replace("\n *", "\n").split())
    for word in ("td_copy_boards", "td_step_boards", "indexed by board id", "byte for byte", "no byte of an unnamed row",
                 "15-B attacker rows", "ledger", "ring guard", "td_kernel_timing", "n == 0", "named twice",
                 "td_frame_skip() > 1", "random_agent = 0", "cap < 0", "TD_LIST_BAD_COUNT", "TD_LIST_RANGE",
                 "TD_LIST_TWICE", "td_list_errors", "status_dev", "count_dev"):
        assert word in doc, word


def test_refusals_that_need_no_handle():
    """td_action_mask's order with the call's own name: a NULL io, the size / abi words, then
    (device form) a negative cap with the io words, then the handle."""
    lib = _lib.lib
    ids = (ctypes.c_int32 * 2)(0, 1)
    calls = {
        "td_action_mask_boards": lambda io, n: lib.td_action_mask_boards(None, io, ids, n, None),
        "td_action_mask_boards_dev": lambda io, n: lib.td_action_mask_boards_dev(None, io, ids, n, None, None, None),
    }
    for name, call in calls.items():
        pre = name.encode()
        assert call(None, 1) < 0 and lib.td_last_error() == pre + b": NULL io"
        io = _lib.TdMaskIO()
        io.abi = 2
        assert call(io, 1) < 0
        assert lib.td_last_error().startswith(pre + b": td_mask_io has size 40 / abi 2"), lib.td_last_error()
        assert call(_lib.TdMaskIO(size=32), 1) < 0 and b"size 32" in lib.td_last_error()
        assert call(_lib.TdMaskIO(), 1) < 0 and lib.td_last_error() == pre + b": NULL handle"
        assert call(_lib.TdMaskIO(), 0) < 0 and lib.td_last_error() == pre + b": NULL handle"
    # cap < 0 needs no handle, but a good io; a bad io is reported first
    assert calls["td_action_mask_boards_dev"](_lib.TdMaskIO(), -1) < 0
    assert lib.td_last_error() == b"td_action_mask_boards_dev: cap = -1 is negative"
    assert calls["td_action_mask_boards_dev"](_lib.TdMaskIO(size=32), -1) < 0 and b"size 32" in lib.td_last_error()
    assert calls["td_action_mask_boards_dev"](None, -1) < 0
    assert lib.td_last_error() == b"td_action_mask_boards_dev: NULL io"
    # td_action_mask's own messages keep td_action_mask's name
    assert lib.td_action_mask(None, None, None) < 0 and lib.td_last_error() == b"td_action_mask: NULL io"
    assert lib.td_action_mask(None, _lib.TdMaskIO(), None) < 0 and lib.td_last_error() == b"td_action_mask: NULL handle"


def test_engine_and_vector_env_say_what_is_fresh():
    from gym_TD import envs
    from gym_TD.engine import TDEngine
    for m, words in ((TDEngine.action_mask_boards, ("td_action_mask_boards", "step_boards", "none twice")),
                     (TDEngine.action_mask_boards_dev, ("td_action_mask_boards_dev", "count", "status", "ValueError"))):
        doc = " ".join(m.__doc__.split())
        assert "only the named rows are fresh" in doc, m.__name__
        for w in words:
            assert w in doc, (m.__name__, w)
    assert "td_action_mask_boards_kernel_name" in TDEngine.action_mask_boards_kernel_name.__doc__
    doc = " ".join(TDEngine.refresh_action_mask.__doc__.split())
    for w in ("action_mask_boards", "written whole", "reset", "config"):
        assert w in doc, w
    for m in (envs.TDVecEnv.fork, envs.TDVecEnv.step_boards, envs.TDVecEnv.fork_dev, envs.TDVecEnv.step_boards_dev):
        assert "action_mask=True" in m.__doc__, m.__name__
