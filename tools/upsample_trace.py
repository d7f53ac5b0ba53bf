#!/usr/bin/env python3
"""From rocprofv3 CSV output (development tool): the k_upsample launches of a pyramidal call, split by grid size (the
per-name --stats summary folds the fine-level launch and the 4x smaller one together).  Reads *kernel_trace.csv for
times and *counter_collection.csv for counters (FETCH_SIZE / WRITE_SIZE in units of 1024 B; FETCH_SIZE is doubled here,
as bench.py's live_traffic does on gfx950).
Usage: python3 tools/upsample_trace.py <dir> [<kernel name part, default k_upsample>]"""
import collections
import csv
import glob
import sys

root = sys.argv[1]
match = sys.argv[2] if len(sys.argv) > 2 else "k_upsample"


def grid_of(r):
    return int(r.get("Grid_Size") or 0) or int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])


times = collections.defaultdict(list)
for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if match in r["Kernel_Name"]:
            times[grid_of(r)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for g in sorted(times, reverse=True):
    t = sorted(times[g])
    print(f"{match} grid {g:>10d} threads: {len(t)} launches, us min {t[0]:.1f} median {t[len(t) // 2]:.1f} "
          f"mean {sum(t) / len(t):.1f} max {t[-1]:.1f}")

ctr = collections.defaultdict(lambda: collections.defaultdict(list))
dur = collections.defaultdict(dict)
for f in glob.glob(root + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if match in r["Kernel_Name"]:
            g = grid_of(r)
            ctr[g][r["Counter_Name"]].append(float(r["Counter_Value"]))
            dur[g][(f, r["Dispatch_Id"])] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
for g in sorted(ctr, reverse=True):
    us = sum(dur[g].values()) / len(dur[g])
    print(f"{match} grid {g:>10d} threads under --pmc: {len(dur[g])} launches, mean {us:.1f} us")
    for c, v in sorted(ctr[g].items()):
        m = sum(v) / len(v)
        if c == "FETCH_SIZE":
            print(f"   FETCH_SIZE x 2 x 1024 B = {m * 2048 / 1e6:.1f} MB per launch, {m * 2048 / us / 1e6:.3f} TB/s")
        elif c == "WRITE_SIZE":
            print(f"   WRITE_SIZE x 1024 B     = {m * 1024 / 1e6:.1f} MB per launch, {m * 1024 / us / 1e6:.3f} TB/s")
        elif c == "GRBM_GUI_ACTIVE":
            print(f"   GRBM_GUI_ACTIVE mean {m:.6g} (/ 8 XCDs / us = {m / 8 / us / 1e3:.3f} GHz)")
        else:
            print(f"   {c} mean {m:.6g}")
