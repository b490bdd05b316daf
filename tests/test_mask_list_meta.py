"""Register / LDS budget of td_mask_list_kernel (td_action_mask_boards, td_action_mask_boards_dev),
read from the gfx950 code object's metadata in libtdstep.so -- no GPU.

The list kernel runs td_mask_kernel's body (td_mask_body.h mask_board), one wave per list entry
and kMaskListWaves entries per workgroup, each wave with an LDS row of its own: so it may cost
kMaskListWaves rows of LDS, no more VGPRs than td_mask_kernel of the same side, and no scratch.
As built: 19 / 23 / 23 / 28 VGPRs at L = 10 / 20 / 30 / generic, the mask kernel's own."""
import os
import re

import pytest

import test_kernel_meta as KM

pytestmark = pytest.mark.skipif(not (KM.TOOLS and os.path.exists(KM.kernel_meta.LIB)),
                                reason="needs the built library and ROCm llvm tools")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = [0, 10, 20, 30]
MAX_KERNEL_L = 32  # td_board.h


def row_bytes(lt):
    """MaskRow<LT>::BYTES (td_mask_body.h): the alignment shift, 6 L^2 + 1 actions, rounded up to 16."""
    nc = lt * lt if lt else MAX_KERNEL_L * MAX_KERNEL_L
    return (15 + 6 * nc + 1 + 15) & ~15


def waves():
    """kMaskListWaves, the build's constant (td_kernels.h)."""
    src = open(os.path.join(ROOT, "gym-td_amd", "csrc", "td_kernels.h")).read()
    m = re.search(r"#define TD_MASK_LIST_WAVES (\d+)", src)
    assert m and "kMaskListWaves = TD_MASK_LIST_WAVES;" in src
    return int(m.group(1))


@pytest.fixture(scope="module")
def meta():
    return KM.kernel_meta.kernels()


def _one(meta, key):
    rows = [r for n, r in meta.items() if key in n]
    assert len(rows) == 1, (key, len(rows))
    return rows[0]


def test_four_list_kernels_and_no_other_shape(meta):
    names = sorted(n for n in meta if "td_mask_list_kernel" in n)
    assert len(names) == 4, names
    want = sorted("_ZN2td19td_mask_list_kernelILi%dEEEvNS_8MaskArgsEPKiiS3_PK14td_list_status" % lt for lt in SIDES)
    assert names == want  # (MaskArgs, ids, cap, count, verdict)


@pytest.mark.parametrize("lt", SIDES)
def test_list_kernel_budget(meta, lt):
    lst = _one(meta, "td_mask_list_kernelILi%dE" % lt)
    full = _one(meta, "td_mask_kernelILi%dE" % lt)
    assert lst.get("scratch", 0) == 0, (lt, lst)
    assert lst["lds"] == waves() * row_bytes(lt), (lt, lst, waves(), row_bytes(lt))
    assert lst["vgpr"] <= full["vgpr"], (lt, lst, full)


@pytest.mark.parametrize("lt", SIDES)
def test_mask_kernels_keep_their_shape(meta, lt):
    """The four td_mask_kernel entries are still there, one LDS row each and no scratch."""
    full = _one(meta, "td_mask_kernelILi%dE" % lt)
    assert full["lds"] == row_bytes(lt) and full.get("scratch", 0) == 0, (lt, full)
    assert len([n for n in meta if "td_mask_kernelI" in n]) == 4


def test_several_entries_per_workgroup():
    assert 2 <= waves() <= 8
