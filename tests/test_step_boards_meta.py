"""Register / LDS budget of the partial-step kernels (td_step_sel_kernel, td_step_boards), read
from the gfx950 code object's metadata in libtdstep.so -- no GPU.

The kernels run the large step kernel's body with the board taken from a list, so each may
cost what td_step_kernel<...> of the same arguments costs and no more: the same LDS, no more
VGPRs, and at most the SGPRs of its two extra kernel parameters on top (a 64-bit pointer and
an int: three, four with the pair's alignment).  Scratch: test_kernel_meta.py's
test_no_kernel_uses_scratch covers every kernel of the library, these included."""
import os

import pytest

import test_kernel_meta as KM

pytestmark = pytest.mark.skipif(not (KM.TOOLS and os.path.exists(KM.kernel_meta.LIB)),
                                reason="needs the built library and ROCm llvm tools")

EXTRA_SGPRS = 4  # const int32_t* ids (an aligned pair), int n
ROWS = [(0, False), (0, True), (1, False), (2, False), (2, True)]  # select_step_kernel's mode / scan rows


@pytest.fixture(scope="module")
def meta():
    return KM.kernel_meta.kernels()


def _one(meta, name, lt, mode, scan):
    key = "%d%sILi%dELi%dELb%dEEEv" % (len(name), name, lt, mode, int(scan))
    rows = [r for n, r in meta.items() if key in n]
    assert len(rows) == 1, (key, len(rows))
    return rows[0]


@pytest.mark.parametrize("fmt", ["", "_f16"])
@pytest.mark.parametrize("lt", [0, 10, 20, 30])
def test_present_and_no_dearer_than_the_large_kernel(meta, lt, fmt):
    for mode, scan in ROWS:
        sel = _one(meta, "td_step_sel_kernel" + fmt, lt, mode, scan)
        large = _one(meta, "td_step_kernel" + fmt, lt, mode, scan)
        assert sel["lds"] == large["lds"], (lt, mode, scan, sel, large)
        assert sel["vgpr"] <= large["vgpr"], (lt, mode, scan, sel, large)
        assert sel["sgpr"] <= large["sgpr"] + EXTRA_SGPRS, (lt, mode, scan, sel, large)
        assert sel.get("scratch", 0) == 0, (lt, mode, scan, sel)


def test_forty_kernels_and_no_other_shape(meta):
    """Five rows x four sides x two formats; no small-batch build of the partial step."""
    names = [n for n in meta if "td_step_sel_kernel" in n]
    assert len(names) == 40, sorted(names)
    assert all(n.endswith("EEEvNS_8StepArgsEPKii") for n in names), sorted(names)
