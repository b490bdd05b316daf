"""Register / LDS budget of the device-list kernels (td_step_list_kernel, td_copy_list_kernel,
td_list_check_kernel: td_step_boards_dev, td_copy_boards_dev), read from the gfx950 code object's
metadata in libtdstep.so -- no GPU.

A list kernel runs td_step_sel_kernel's body behind two wave-uniform loads, so each may cost
what the sel kernel of the same arguments costs: the same LDS, no more VGPRs, no scratch, and at
most the SGPRs of its two added 64-bit pointers on top (as built: not one more in any row)."""
import os

import pytest

import test_kernel_meta as KM

pytestmark = pytest.mark.skipif(not (KM.TOOLS and os.path.exists(KM.kernel_meta.LIB)),
                                reason="needs the built library and ROCm llvm tools")

EXTRA_SGPRS = 4  # const int32_t* count, const td_list_status* verdict
ROWS = [(0, False), (0, True), (1, False), (2, False), (2, True)]  # select_row's mode / scan rows
SIDES = [0, 10, 20, 30]


@pytest.fixture(scope="module")
def meta():
    return KM.kernel_meta.kernels()


def _one(meta, key):
    rows = [r for n, r in meta.items() if key in n]
    assert len(rows) == 1, (key, len(rows))
    return rows[0]


def _step(meta, name, lt, mode, scan):
    return _one(meta, "%d%sILi%dELi%dELb%dEEEv" % (len(name), name, lt, mode, int(scan)))


@pytest.mark.parametrize("fmt", ["", "_f16"])
@pytest.mark.parametrize("lt", SIDES)
def test_step_list_kernels_present_and_no_dearer_than_the_sel_kernels(meta, lt, fmt):
    for mode, scan in ROWS:
        lst = _step(meta, "td_step_list_kernel" + fmt, lt, mode, scan)
        sel = _step(meta, "td_step_sel_kernel" + fmt, lt, mode, scan)
        assert lst["lds"] == sel["lds"], (lt, mode, scan, lst, sel)
        assert lst["vgpr"] <= sel["vgpr"], (lt, mode, scan, lst, sel)
        assert lst["sgpr"] <= sel["sgpr"] + EXTRA_SGPRS, (lt, mode, scan, lst, sel)
        assert lst.get("scratch", 0) == 0, (lt, mode, scan, lst)


def test_forty_step_list_kernels_and_no_other_shape(meta):
    """Five rows x four sides x two formats, each (StepArgs, ids, cap, count, verdict)."""
    names = [n for n in meta if "td_step_list_kernel" in n]
    assert len(names) == 40, sorted(names)
    assert all(n.endswith("EEEvNS_8StepArgsEPKiiS3_PK14td_list_status") for n in names), sorted(names)
    assert not any("td_step_sel_kernel" in n for n in names)


@pytest.mark.parametrize("lt", SIDES)
def test_copy_list_kernel_per_side_no_dearer_than_the_copy_kernel(meta, lt):
    lst = _one(meta, "td_copy_list_kernelILi%dE" % lt)
    cpy = _one(meta, "td_copy_kernelILi%dE" % lt)
    assert lst["lds"] == cpy["lds"], (lt, lst, cpy)
    assert lst["vgpr"] <= cpy["vgpr"], (lt, lst, cpy)
    assert lst["sgpr"] <= cpy["sgpr"] + EXTRA_SGPRS, (lt, lst, cpy)
    assert lst.get("scratch", 0) == 0, (lt, lst)


def test_check_kernel_uses_no_scratch_and_no_lds(meta):
    """td_list_check_kernel declares no LDS at all: the last block's work is one thread's."""
    chk = _one(meta, "td_list_check_kernel")
    assert chk.get("scratch", 0) == 0 and chk["lds"] == 0, chk
    assert chk["vgpr"] <= 32 and chk["sgpr"] <= 48, chk  # (10 / 29 as built: nothing that limits occupancy)
