#!/usr/bin/env python3
"""Per (kernel, grid size) launch statistics from a `rocprofv3 --kernel-trace --output-format csv` trace.

`--stats` groups by kernel name alone; the coarse and the fine launch of the fused MLP kernel share a name and differ in their
grid, so this table is what separates them.  usage: trace_by_grid.py <*_kernel_trace.csv> [top N, default 12]"""
import csv
import statistics as st
import sys


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    cut = name.find("(")
    return (name if cut < 0 else name[:cut])[-64:]


def main(path, top=12):
    groups = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            groups.setdefault((short(r["Kernel_Name"]), int(r["Grid_Size_X"])), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    print(f"{'kernel':64s} {'grid x':>9s} {'calls':>6s} {'mean us':>10s} {'median us':>10s} {'min us':>10s} {'max us':>10s}")
    for (name, grid), v in sorted(groups.items(), key=lambda kv: -sum(kv[1]))[:top]:
        print(f"{name:64s} {grid:9d} {len(v):6d} {st.mean(v) / 1e3:10.2f} {st.median(v) / 1e3:10.2f} {min(v) / 1e3:10.2f} {max(v) / 1e3:10.2f}")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 12)
