"""Register / LDS budget of td_sample_weighted_kernel (td_sample_weighted and its list forms), read
from the gfx950 code object's metadata in libtdstep.so -- no GPU.

td_sample_kernel's shape: one wave per entry and kSampleWaves entries per workgroup, each wave
with the uniform sampler's LDS row (the 6 L^2 fail codes rounded up to 16 B; the no-op has no
byte in it, the sums run on lane shuffles).  No scratch.  The registers stand in DESIGN.md's
table, recorded, not fixed in advance.  The uniform sampler and the mask kernels keep their shape."""
import os
import re

import pytest

import test_kernel_meta as KM
import test_mask_list_meta as MLM
import test_sample_meta as SM

pytestmark = pytest.mark.skipif(not (KM.TOOLS and os.path.exists(KM.kernel_meta.LIB)),
                                reason="needs the built library and ROCm llvm tools")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = [0, 10, 20, 30]


@pytest.fixture(scope="module")
def meta():
    return KM.kernel_meta.kernels()


def test_exactly_four_weighted_kernels(meta):
    names = sorted(n for n in meta if "td_sample_weighted_kernel" in n)
    want = sorted("_ZN2td25td_sample_weighted_kernelILi%dEEEvNS_11SampleWArgsEPKiiS3_PK14td_list_status" % lt for lt in SIDES)
    assert names == want  # (SampleWArgs, ids, cap, count, verdict)


@pytest.mark.parametrize("lt", SIDES)
def test_weighted_kernel_budget(meta, lt):
    k = MLM._one(meta, "td_sample_weighted_kernelILi%dE" % lt)
    uni = MLM._one(meta, "td_sample_kernelILi%dE" % lt)
    assert k.get("scratch", 0) == 0, (lt, k)
    assert k["lds"] == SM.waves() * SM.row_bytes(lt), (lt, k, SM.waves(), SM.row_bytes(lt))
    assert k["lds"] <= uni["lds"]  # no more than the uniform sampler's per workgroup
    # the formula as the kernel's file states it
    src = open(os.path.join(ROOT, "gym-td_amd", "csrc", "td_sample_w.hip")).read()
    assert "LDS = kSampleWaves * SampleWRow<L>::BYTES" in src
    assert "{:,}".format(SM.waves() * SM.row_bytes(lt)) in src


def test_design_table_states_the_figures(meta):
    """DESIGN.md section 4 "Sampling from weights": one row per kernel, | L | SGPR | VGPR | LDS |."""
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = doc.index("### Sampling from weights")
    sec = doc[at:doc.index("\n### ", at + 1)]
    rows = {m.group(1): tuple(int(x.replace(",", "")) for x in m.group(2, 3, 4))
            for m in re.finditer(r"^\| (10|20|30|generic) \| (\d+) \| (\d+) \| ([\d,]+) \|", sec, re.M)}
    assert len(rows) == 4, sorted(rows)
    for lt in SIDES:
        k = MLM._one(meta, "td_sample_weighted_kernelILi%dE" % lt)
        assert rows[str(lt) if lt else "generic"] == (k["sgpr"], k["vgpr"], k["lds"]), (lt, k)


@pytest.mark.parametrize("lt", SIDES)
def test_uniform_sampler_and_mask_kernels_are_still_there(meta, lt):
    uni = MLM._one(meta, "td_sample_kernelILi%dE" % lt)
    assert uni["lds"] == SM.waves() * SM.row_bytes(lt) and uni.get("scratch", 0) == 0
    full = MLM._one(meta, "td_mask_kernelILi%dE" % lt)
    lst = MLM._one(meta, "td_mask_list_kernelILi%dE" % lt)
    assert full["lds"] == MLM.row_bytes(lt) and lst["lds"] == MLM.waves() * MLM.row_bytes(lt)
    assert len([n for n in meta if "td_sample_kernelI" in n]) == 4
    assert len([n for n in meta if "td_mask_kernelI" in n]) == 4
    assert len([n for n in meta if "td_mask_list_kernelI" in n]) == 4
