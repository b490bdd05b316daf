"""Register / LDS budget of td_probe_kernel (td_probe and its list forms), read from the gfx950
code object's metadata in libtdstep.so -- no GPU.

One wave per (entry, replica) and one board image per workgroup: the playout's image and raw cell
words and, in TD-def and TD-atk, the replica's private copy of the opponent's stream (624 words;
td_probe.h).  Twelve kernels -- L = 10 / 20 / 30 and the generic build, three modes --, none with
scratch; their figures stand in DESIGN.md's table, recorded, not fixed in advance."""
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
MT_BYTES = 624 * 4


@pytest.fixture(scope="module")
def meta():
    return KM.kernel_meta.kernels()


def _kernel(meta, lt, mode):
    return MLM._one(meta, "td_probe_kernelILi%dELi%dEE" % (lt, mode))


def test_exactly_twelve_probe_kernels(meta):
    names = sorted(n for n in meta if "td_probe_kernel" in n)
    want = sorted("_ZN2td15td_probe_kernelILi%dELi%dEEEvNS_8StepArgsENS_9ProbeArgsE" % (lt, m)
                  for lt in SIDES for m in MODES)
    assert names == want  # (StepArgs unchanged in front, ProbeArgs behind it)
    assert not any("td_playout_kernel" in n for n in names)  # (the playout's census counts by that substring)


@pytest.mark.parametrize("lt", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_no_scratch_and_the_stream_beside_the_playouts_image(meta, lt, mode):
    k = _kernel(meta, lt, mode)
    assert k.get("scratch", 0) == 0, (lt, mode, k)
    playout = MLM._one(meta, "td_playout_kernelILi%dELi%dEE" % (lt, mode))
    # the playout's workgroup, plus the private stream where the mode has a built-in opponent
    assert k["lds"] == playout["lds"] + (0 if mode == 2 else MT_BYTES), (lt, mode, k["lds"], playout["lds"])
    assert k["lds"] <= 64 * 1024


def test_design_table_states_the_figures(meta):
    """DESIGN.md section 4 "Probes": one row per kernel, | L | mode | SGPR | VGPR | LDS |."""
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = doc.index("### Probes")
    assert at > doc.index("\n### ", doc.index("### Playouts") + 1)  # a section of its own, not inside "Playouts"
    nxt = re.search(r"\n##+ ", doc[at + 1:])
    sec = doc[at:at + 1 + nxt.start()] if nxt else doc[at:]
    rows = {(m.group(1), m.group(2)): tuple(int(x.replace(",", "")) for x in m.group(3, 4, 5))
            for m in re.finditer(r"^\| (10|20|30|generic) \| (TD-def|TD-atk|TD-2p) \| (\d+) \| (\d+) \| ([\d,]+) \|", sec, re.M)}
    assert len(rows) == 12, sorted(rows)
    for lt in SIDES:
        for mode, name in zip(MODES, ("TD-def", "TD-atk", "TD-2p")):
            k = _kernel(meta, lt, mode)
            assert rows[(str(lt) if lt else "generic", name)] == (k["sgpr"], k["vgpr"], k["lds"]), (lt, name, k)
