"""The ring fit's set-up in a rocprofv3 --kernel-trace CSV of bench.py (profiles/fit_setup/README.md): per iteration -- from one k_ring_pmax, the kernel a
background fit ends with, to the next -- the k_pin_copy dispatches and their summed time, the window projection's duration, the span from its start to the start of
the ring solve, and the kernels that STARTED inside the projection's interval (with option fit_side = 1 these are the fit's set-up on the side stream; on one stream
there are none).

    python scripts/fit_setup_trace.py <kernel_trace.csv> [iterations from the end, default 2]"""
import csv
import sys


def short(n):
    return n.split("(")[0].replace("void ", "").replace("cnmfe::", "")[:48]


def main():
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(sys.argv[1]))), key=lambda x: x[0])
    nit = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    marks = [i for i, r in enumerate(rows) if "k_ring_pmax" in r[2]]
    for a, b in list(zip(marks[:-1], marks[1:]))[-nit:]:
        it = rows[a + 1:b + 1]
        pins = [r for r in it if "k_pin_copy" in r[2]]
        proj = [r for r in it if "k_win_proj" in r[2]]
        solve = [r for r in it if "k_ring_solve" in r[2]]
        span = (max(r[1] for r in it) - it[0][0]) / 1e6
        busy = sum(e - s for s, e, _ in it) / 1e6
        print("iteration: %d kernels, span %.3f ms, summed kernel time %.3f ms" % (len(it), span, busy))
        print("  k_pin_copy: %d dispatches, %.3f ms in all" % (len(pins), sum(e - s for s, e, _ in pins) / 1e6))
        if not proj or not solve:
            print("  (no window projection / ring solve in this iteration)")
            continue
        p0, p1 = proj[0][0], max(r[1] for r in proj)
        print("  window projection: %d launches, %.3f ms from its start to its end" % (len(proj), (p1 - p0) / 1e6))
        print("  start of the projection -> start of the ring solve: %.3f ms" % ((solve[0][0] - p0) / 1e6))
        between = [r for r in it if p0 <= r[0] < solve[0][0] and r not in proj]
        print("  kernels between the two starts: %d, %.3f ms summed" % (len(between), sum(e - s for s, e, _ in between) / 1e6))
        inside = [r for r in it if p0 < r[0] < p1 and r not in proj]
        print("  started inside the projection's interval: %d kernels, %.3f ms summed" % (len(inside), sum(e - s for s, e, _ in inside) / 1e6))
        for s, e, n in inside:
            print("    +%8.1f us  %7.1f us  %s" % ((s - p0) / 1e3, (e - s) / 1e3, short(n)))


if __name__ == "__main__":
    main()
