"""The spatial -> temporal hand-over in a rocprofv3 --kernel-trace CSV, per iteration (iterations delimited like scripts/gap_analysis.py):
   python scripts/handover_gaps.py <kernel_trace.csv>
 * idle (the sum of the gaps between consecutive kernels) from the end of k_connectivity to the first temporal projection dispatch (k_vp_proj_*),
 * idle from the end of k_ata_pairs to the first k_hals_temporal dispatch,
 * the durations of k_vp_build_b, k_vp_bdig, the projection, k_vp_reduce and k_vp_const,
 * the iteration's span, busy time and idle."""
import csv, sys
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(sys.argv[1]))), key=lambda x: x[0])
idx = [i for i, r in enumerate(rows) if "k_ring_pmax" in r[2]]
NAMES = ("k_vp_build_b", "k_vp_bdig", "k_vp_proj_i8", "k_vp_proj_b", "k_vp_reduce", "k_vp_const", "k_keep_values", "k_aa_gather")


def idle(it, a, b):
    """sum of the gaps between consecutive kernels from the end of it[a] to the start of it[b]"""
    return sum(max(0, it[i + 1][0] - max(e for _, e, _ in it[a:i + 1])) for i in range(a, b)) / 1e6


def first(it, name, start=0):
    return next((i for i in range(start, len(it)) if name in it[i][2]), None)


for n in range(len(idx) - 1):
    it = rows[idx[n]:idx[n + 1]]
    span = (it[-1][1] - it[0][0]) / 1e6
    busy = sum(e - s for s, e, _ in it) / 1e6
    c = first(it, "k_connectivity")
    p = first(it, "k_vp_proj", c or 0) if c is not None else None
    a = first(it, "k_ata_pairs")
    h = first(it, "k_hals_temporal", a or 0) if a is not None else None
    dur = {k: sum(e - s for s, e, nm in it if k in nm) / 1e6 for k in NAMES}
    print("iteration %d: span %.3f ms, busy %.3f ms, idle %.3f ms, %d kernels" % (n, span, busy, idle(it, 0, len(it) - 1), len(it)))
    if c is not None and p is not None:
        print("   idle k_connectivity -> first temporal projection: %.3f ms (interval %.3f ms)" % (idle(it, c, p), (it[p][0] - it[c][1]) / 1e6))
    if a is not None and h is not None:
        print("   idle k_ata_pairs -> first k_hals_temporal:        %.3f ms (interval %.3f ms)" % (idle(it, a, h), (it[h][0] - it[a][1]) / 1e6))
    print("   " + "  ".join("%s %.3f" % (k, v) for k, v in dur.items() if v > 0) + "  (ms)")
