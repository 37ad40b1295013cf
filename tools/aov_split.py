#!/usr/bin/env python3
"""Where one rrt_render_aov call spends its time, from a rocprofv3 --kernel-trace CSV of tools/aov_time.py (whose last call is a feature-buffer pass
over all samples): the dispatches from the last camera-kernel launch to the end of the trace, summed by family.

    rocprofv3 --kernel-trace --stats --output-format csv -d results/aov_prof -- python3 tools/aov_time.py 3
    python tools/aov_split.py results/aov_prof
"""
import csv
import glob
import sys

f = sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True))[0]
rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
first = [i for i, r in enumerate(rows) if "k_pixel_offsets" in r["Kernel_Name"] or "k_raygen<" in r["Kernel_Name"]][-1]
FAMILIES = (("camera", ("k_pixel_offsets", "k_raygen")), ("traversal", ("k_trace_", "k_closest", "k_tt_snapshot")), ("k_aov_shade", ("k_aov_shade",)),
            ("film", ("k_gather_box", "k_gather_wide")), ("merge", ("k_aov_merge",)))
total = {}
for r in rows[first:]:
    name = r["Kernel_Name"]
    fam = next((k for k, keys in FAMILIES if any(s in name for s in keys)), "other")
    total[fam] = total.get(fam, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
span = (int(rows[-1]["End_Timestamp"]) - int(rows[first]["Start_Timestamp"])) / 1e6
print("last rrt_render_aov call, kernel time by family (ms): " + ", ".join(f"{k} {v:.3f}" for k, v in total.items()) + f" | first launch to last end {span:.3f}")
