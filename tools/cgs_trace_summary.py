"""k_cgs launches of a rocprofv3 kernel trace, grouped by launch grid.

    python tools/cgs_trace_summary.py <..._kernel_trace.csv> [--min-us 15]

One line per grid (strips x bands, in blocks): launches, the active ones
(launches enqueued after convergence return after their prologue; they are
told apart by duration), and median / mean / total duration of the active
launches.
"""
import argparse
import csv
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--min-us", type=float, default=15.0, help="shortest launch counted as active")
    ap.add_argument("--kernel", default="k_cgs")
    args = ap.parse_args()
    by = {}
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            if args.kernel not in r["Kernel_Name"]:
                continue
            gx = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
            gy = int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"]))
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
            by.setdefault((gx, gy), []).append(us)
    if not by:
        sys.exit(f"no {args.kernel} launch in {args.trace}")
    for (gx, gy), d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        act = [u for u in d if u >= args.min_us] or d
        print(f"blocks {gx}x{gy}: {len(d)} launches, {len(act)} active (>= {args.min_us:g} us): "
              f"median {statistics.median(act):.1f} us mean {statistics.fmean(act):.1f} us "
              f"total {sum(act) * 1e-3:.1f} ms")


if __name__ == "__main__":
    main()
