"""Register / LDS budget of td_sample_kernel (td_sample_actions and its list forms), read from the
gfx950 code object's metadata in libtdstep.so -- no GPU.

One wave per entry and kSampleWaves entries per workgroup, each wave with an LDS row of its own:
the 6 L^2 fail codes rounded up to 16 B (td_sample.hip SampleRow; the prefix sum runs on lane
shuffles and takes no LDS).  No scratch.  The mask kernels beside it keep their shape."""
import os
import re

import pytest

import test_kernel_meta as KM
import test_mask_list_meta as MLM

pytestmark = pytest.mark.skipif(not (KM.TOOLS and os.path.exists(KM.kernel_meta.LIB)),
                                reason="needs the built library and ROCm llvm tools")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = [0, 10, 20, 30]
MAX_KERNEL_L = 32  # td_board.h


def row_bytes(lt):
    """SampleRow<LT>::BYTES (td_sample.hip): 6 L^2 codes, rounded up to 16."""
    nc = lt * lt if lt else MAX_KERNEL_L * MAX_KERNEL_L
    return (6 * nc + 15) & ~15


def waves():
    """kSampleWaves (td_kernels.h)."""
    m = re.search(r"constexpr int kSampleWaves = (\d+);", open(os.path.join(ROOT, "gym-td_amd", "csrc", "td_kernels.h")).read())
    assert m
    return int(m.group(1))


@pytest.fixture(scope="module")
def meta():
    return KM.kernel_meta.kernels()


def test_exactly_four_sample_kernels(meta):
    names = sorted(n for n in meta if "td_sample_kernel" in n)
    want = sorted("_ZN2td16td_sample_kernelILi%dEEEvNS_10SampleArgsEPKiiS3_PK14td_list_status" % lt for lt in SIDES)
    assert names == want  # (SampleArgs, ids, cap, count, verdict)
    assert not any("td_mask_kernel" in n or "td_mask_list_kernel" in n for n in names)


@pytest.mark.parametrize("lt", SIDES)
def test_sample_kernel_budget(meta, lt):
    k = MLM._one(meta, "td_sample_kernelILi%dE" % lt)
    assert k.get("scratch", 0) == 0, (lt, k)
    assert k["lds"] == waves() * row_bytes(lt), (lt, k, waves(), row_bytes(lt))
    assert k["lds"] <= 64 * 1024
    # the formula as the kernel's file states it
    src = open(os.path.join(ROOT, "gym-td_amd", "csrc", "td_sample.hip")).read()
    assert "LDS = kSampleWaves * SampleRow<L>::BYTES" in src
    assert "{:,}".format(waves() * row_bytes(lt)) in src


@pytest.mark.parametrize("lt", SIDES)
def test_mask_kernels_are_still_there(meta, lt):
    full = MLM._one(meta, "td_mask_kernelILi%dE" % lt)
    lst = MLM._one(meta, "td_mask_list_kernelILi%dE" % lt)
    assert full["lds"] == MLM.row_bytes(lt) and lst["lds"] == MLM.waves() * MLM.row_bytes(lt)
    assert len([n for n in meta if "td_mask_kernelI" in n]) == 4
    assert len([n for n in meta if "td_mask_list_kernelI" in n]) == 4
