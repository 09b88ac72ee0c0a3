#!/usr/bin/env python3
"""Summarise PMC-only rocprofv3 passes of `python bench.py --serial --steps 1` for the JL
exponentiation launch (jl_exp_kernel<true>) into profiles/.

    python tools/exp_boundary_pmc.py DIR OUT.json [kernel_trace_dir]

DIR holds one sub-directory per pass (pmc1, pmc2, ...: `rocprofv3 --pmc COUNTERS --output-format csv -d
DIR/pmcK -o run -- python bench.py --serial --steps 1`, counters alone, no tracing in the same run); every
dispatch of the kernel is listed with its counters.  Derived, per pass that has the counters (as
profiles/archive/r3_single_sq_counters.json): SIMD cycles = GRBM_GUI_ACTIVE / XCDs, VALU instructions per
SIMD = SQ_INSTS_VALU / (CUs x 4), the VALU issue fraction = 4 clocks x VALU instructions per SIMD / SIMD
cycles (a wave64 VALU instruction holds its SIMD's issue port 4 clocks; v_mad_u64_u32 more -- the fraction
counts slots, not time), LDS instructions per launch and the wait counters as fractions of the wave cycles.
"""

import collections
import csv
import glob
import json
import os
import sys

KERNEL = "jl_exp_kernel<true>"
XCDS, CUS = 8, 256


def dispatches(d):
    out = collections.OrderedDict()
    for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if KERNEL in r["Kernel_Name"]:
                    e = out.setdefault(r["Dispatch_Id"], {"dispatch": r["Dispatch_Id"],
                                                          "ms": (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6})
                    e[r["Counter_Name"]] = e.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    return list(out.values())


def main(src, dst, trace=None):
    res = {"meta": f"PMC-only rocprofv3 passes of `python bench.py --serial --steps 1` (10M elements, 8 parties), "
                   f"{KERNEL}: counters alone in each run; GRBM counts summed over the {XCDS} XCDs",
           "dispatches": [], "derived": {}}
    for p in sorted(os.listdir(src)):
        if not (p.startswith("pmc") and os.path.isdir(os.path.join(src, p))):
            continue
        for e in dispatches(os.path.join(src, p)):
            res["dispatches"].append(dict(e, **{"pass": p}))
    full = [e for e in res["dispatches"] if "SQ_INSTS_VALU" in e and "GRBM_GUI_ACTIVE" in e]
    if full:
        e = full[-1]  # the measured step (the first dispatch is the warm-up)
        cyc, valu = e["GRBM_GUI_ACTIVE"] / XCDS, e["SQ_INSTS_VALU"] / (CUS * 4)
        der = {"dispatch": e["dispatch"], "launch_ms_under_pmc": e["ms"], "cycles_per_simd": cyc,
               "clock_GHz_from_GRBM": cyc / e["ms"] / 1e6, "valu_instr_per_simd": valu,
               "clk_per_valu_instr": cyc / valu, "valu_issue_fraction_4clk": 4.0 * valu / cyc,
               "lds_instr_per_launch": e.get("SQ_INSTS_LDS")}
        for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_ANY"):
            if k in e and e.get("SQ_WAVE_CYCLES"):
                der[k + "_per_wave_cycle"] = e[k] / e["SQ_WAVE_CYCLES"]
        res["derived"] = der
    second = [e for e in res["dispatches"] if "SQ_WAIT_INST_LDS" in e]
    if second:
        e = second[-1]
        res["derived"].update({"SQ_WAIT_INST_LDS": e["SQ_WAIT_INST_LDS"], "SQ_ACTIVE_INST_LDS": e.get("SQ_ACTIVE_INST_LDS"),
                               "SQ_INSTS_SMEM": e.get("SQ_INSTS_SMEM"), "SQ_INSTS_SALU": e.get("SQ_INSTS_SALU"),
                               "SQ_BUSY_CYCLES": e.get("SQ_BUSY_CYCLES")})
    if trace:
        ms = []
        for f in glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True):
            with open(f) as fh:
                ms += [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in csv.DictReader(fh)
                       if KERNEL in r["Kernel_Name"]]
        if ms:
            res["trace_launch_ms"] = ms
            res["derived"]["launch_ms_trace_median"] = sorted(ms)[len(ms) // 2]
    with open(dst, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["derived"], indent=1))


if __name__ == "__main__":
    main(*sys.argv[1:4])
