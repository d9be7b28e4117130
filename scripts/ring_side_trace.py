"""The last iteration of a rocprofv3 --kernel-trace CSV of bench.py, from the end of one ring solve to the end of the next: per kernel its start relative to the end of
the first solve, its duration, its queue and its name (profiles/trace_ahead/README.md: with option ring_side the ring statistics and the W*A tables start on a
second queue inside the spatial update's interval).

    python scripts/ring_side_trace.py <kernel_trace.csv>"""
import csv
import sys


def main():
    rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
    qcol = next((c for c in ("Queue_Id", "Stream_Id", "Queue_ID") if c in rows[0]), None)
    solves = [i for i, r in enumerate(rows) if "k_ring_solve" in r["Kernel_Name"]]
    a = solves[-2]
    t0 = int(rows[a]["End_Timestamp"])
    print("columns:", list(rows[0].keys()))
    for r in rows[a:solves[-1] + 1]:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        print("%9.1f us  %8.1f us  q=%s  %s" % ((s - t0) / 1e3, (e - s) / 1e3, r.get(qcol, "?") if qcol else "?", r["Kernel_Name"].split("(")[0][:60]))


if __name__ == "__main__":
    main()
