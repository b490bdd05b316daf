"""VALU busy of the step kernel from one rocprofv3 --pmc pass over bench.py.

    rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY \\
        SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_WAVE_CYCLES GRBM_GUI_ACTIVE -d DIR -o pmc --output-format csv -- python bench.py ...
    python scripts/pmc_valu_busy.py DIR OUT.json

Per launch of the most frequent td_step_kernel* (means over its dispatches).  rocprofv3 reports
GRBM_GUI_ACTIVE summed over the 8 XCDs, so the kernel lasts GRBM_GUI_ACTIVE / 8 shader cycles;
SQ_ACTIVE_INST_VALU counts in units of 4 cycles, summed over the 1,024 SIMDs:

    VALU busy = 4 * SQ_ACTIVE_INST_VALU / 1024 / (GRBM_GUI_ACTIVE / 8)
"""
import collections
import csv
import glob
import json
import sys

XCDS, SIMDS = 8, 1024


def main():
    d, out = sys.argv[1], sys.argv[2]
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    ids = collections.defaultdict(set)
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "td_step_kernel" not in r["Kernel_Name"]:
                continue
            k = r["Kernel_Name"].split("(")[0]
            per[k][r["Counter_Name"]] += float(r["Counter_Value"])
            ids[k].add(r["Dispatch_Id"])
    if not per:
        raise SystemExit("no td_step_kernel dispatch under " + d)
    kern = max(ids, key=lambda k: len(ids[k]))
    n = len(ids[kern])
    c = {name: v / n for name, v in per[kern].items()}
    res = {"kernel": kern, "launches": n, "per_launch": c}
    cyc = c["GRBM_GUI_ACTIVE"] / XCDS
    res["kernel_cycles"] = cyc
    if "SQ_ACTIVE_INST_VALU" in c:
        res["valu_busy"] = 4.0 * c["SQ_ACTIVE_INST_VALU"] / SIMDS / cyc
    if "SQ_WAVES" in c:
        for name in ("SQ_INSTS_VALU", "SQ_INSTS_SALU"):
            if name in c:
                res[name.lower() + "_per_wave"] = c[name] / c["SQ_WAVES"]
    if "SQ_WAVE_CYCLES" in c:
        for name in ("SQ_WAIT_INST_ANY", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_ANY"):
            if name in c:
                res[name.lower() + "_of_wave_cycles"] = c[name] / c["SQ_WAVE_CYCLES"]
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
