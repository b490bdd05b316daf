"""Register / LDS budget of td_playout_kernel (td_playout and its list forms), read from the
gfx950 code object's metadata in libtdstep.so -- no GPU.

One wave per entry and one board per workgroup: the board image (Smem) and, beside it, the raw
cell words (td_playout.h).  Twelve kernels -- L = 10 / 20 / 30 and the generic build, three modes
--, none with scratch; their figures stand in DESIGN.md's table, recorded, not fixed in advance."""
import os
import re

import pytest

import test_kernel_meta as KM
import test_mask_list_meta as MLM

pytestmark = pytest.mark.skipif(not (KM.TOOLS and os.path.exists(KM.kernel_meta.LIB)),
                                reason="needs the built library and ROCm llvm tools")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = [0, 10, 20, 30]
MODES = [0, 1, 2]
MAX_KERNEL_L = 32  # td_board.h


@pytest.fixture(scope="module")
def meta():
    return KM.kernel_meta.kernels()


def _kernel(meta, lt, mode):
    return MLM._one(meta, "td_playout_kernelILi%dELi%dEE" % (lt, mode))


def test_exactly_twelve_playout_kernels(meta):
    names = sorted(n for n in meta if "td_playout_kernel" in n)
    want = sorted("_ZN2td17td_playout_kernelILi%dELi%dEEEvNS_8StepArgsENS_11PlayoutArgsE" % (lt, m)
                  for lt in SIDES for m in MODES)
    assert names == want  # (StepArgs unchanged in front, PlayoutArgs behind it)


@pytest.mark.parametrize("lt", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_no_scratch_and_the_raw_cells_beside_the_board(meta, lt, mode):
    k = _kernel(meta, lt, mode)
    assert k.get("scratch", 0) == 0, (lt, mode, k)
    nc = lt * lt if lt else MAX_KERNEL_L * MAX_KERNEL_L
    # the frame-skip kernel of the same side: TD-atk keeps the raw words too, the other modes none
    skip = MLM._one(meta, "td_skip_kernelILi%dELi%dEE" % (lt, mode))
    assert k["lds"] == skip["lds"] + (0 if mode == 1 else 4 * nc), (lt, mode, k["lds"], skip["lds"])
    assert k["lds"] <= 64 * 1024


def test_design_table_states_the_figures(meta):
    """DESIGN.md section 4 "Playouts": one row per kernel, | L | mode | SGPR | VGPR | LDS |."""
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = doc.index("### Playouts")
    sec = doc[at:doc.index("\n### ", at + 1)]
    rows = {(m.group(1), m.group(2)): tuple(int(x.replace(",", "")) for x in m.group(3, 4, 5))
            for m in re.finditer(r"^\| (10|20|30|generic) \| (TD-def|TD-atk|TD-2p) \| (\d+) \| (\d+) \| ([\d,]+) \|", sec, re.M)}
    assert len(rows) == 12, sorted(rows)
    for lt in SIDES:
        for mode, name in zip(MODES, ("TD-def", "TD-atk", "TD-2p")):
            k = _kernel(meta, lt, mode)
            assert rows[(str(lt) if lt else "generic", name)] == (k["sgpr"], k["vgpr"], k["lds"]), (lt, name, k)
