#!/usr/bin/env python3
"""SQ counters of trace_synth_kernel (csrc/abr_env.hip), in a rocprofv3 --pmc pass of its own.

    rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES \
        --output-format csv -d DIR -- python tools/trace_synth_counters.py
    python tools/trace_synth_counters.py --aggregate DIR OUT.json

Without arguments: five abr_trace_synth launches for each corpus shape and K of tools/bench_trace_synth.py (1 024 x 1 000
then 16 384 x 1 000, K = 4 then 8), nothing else on the device.  --aggregate: every trace_synth_kernel row of DIR's
counter_collection CSVs, by grid size in threads (65 536 = 1 024 traces, 524 288 = the 2 048-workgroup cap), each
counter's values in launch order, written to OUT.json (profiles/trace_synth_sq_counters.json is such a file)."""
import collections
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PMC = "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES"


def launches():
    import torch
    import abrsimulator_amd as A
    import bench_trace_synth as B
    for (n, length) in B.SHAPES:
        for K, kw in B.MODELS.items():
            m = A.TraceModel(**kw)
            out = A.synth_traces(m, [length] * n, B.SEED)
            for g in range(4):
                A.synth_traces(m, None, B.SEED, generation=g, out=out)
            torch.cuda.synchronize()


def aggregate(root, out_path):
    rows = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in sorted(glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            if "trace_synth_kernel" in r["Kernel_Name"]:
                rows[int(r["Grid_Size"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
    res = {"command": f"rocprofv3 --pmc {PMC} --output-format csv -d DIR -- python tools/trace_synth_counters.py; "
                      "python tools/trace_synth_counters.py --aggregate DIR OUT.json",
           "launch_order": "per grid size: five launches at K = 4, then five at K = 8",
           "by_grid_size_threads": {str(g): dict(d) for g, d in sorted(rows.items())}}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--aggregate":
        aggregate(sys.argv[2], sys.argv[3])
    else:
        launches()
