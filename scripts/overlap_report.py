"""usage: python scripts/overlap_report.py <rocprofv3 output dir>

For every fork site of a major iteration -- the weight image's k_boxw beside the data image's kernel, the time medians of
the residual beside its transpose -- how much of the shorter kernel's interval lies inside the longer one's, from the
timestamps of a rocprofv3 --kernel-trace run of bench.py.  A pair is a dispatch of the first kernel and the next dispatch
of its partner.  wall = first start to last end of the pair; serial = the sum of the two durations.
"""
import collections
import csv
import glob
import os
import sys

# (site, first kernel prefix, partner prefixes)
SITES = [("P1 k_boxw<108> | k_boxq_deep<96, 1>", "k_boxw<108>", ("k_boxq_deep<96, 1>",)),
         ("P1 k_boxw<86>  | k_boxq<80, 1, 8>", "k_boxw<86>", ("k_boxq<80, 1, 8>",)),
         ("P1 k_boxw<64>  | k_boxq<64, 1, 8>", "k_boxw<64>", ("k_boxq<64, 1, 8>",)),
         ("P1 k_boxw<42>  | k_boxt<32, true, 1>", "k_boxw<42>", ("k_boxt<32, true, 1>",)),
         ("P1 k_boxw<20>  | k_boxt<20, false, 1>", "k_boxw<20>", ("k_boxt<20, false, 1>",)),
         ("P2 k_transpose<float, true> | k_median_wave<16, true, 1>", "k_transpose<float, true>", ("k_median_wave<16, true, 1>",))]


def name_of(row):
    n = row["Kernel_Name"].split("(")[0]
    return n[5:] if n.startswith("void ") else n


def main(directory):
    fn = max(glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True), key=os.path.getmtime)
    rows = [r for r in csv.DictReader(open(fn)) if name_of(r).startswith("k_")]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]) if r.get("Dispatch_Id") else int(r["Start_Timestamp"]))
    ev = [(name_of(r), int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
    # only the slab-sized launches (the spectrum path has small ones of the same kernels)
    longest = collections.defaultdict(int)
    for n, s, e in ev:
        longest[n] = max(longest[n], e - s)
    print("trace:", os.path.basename(fn), " kernels:", len(ev))
    print("%-58s %5s %9s %9s %9s %8s %9s %9s" % ("site", "pairs", "first_ms", "partn_ms", "overl_ms", "of short", "wall_ms", "serial_ms"))
    for site, first, partners in SITES:
        acc = []
        for i, (n, s, e) in enumerate(ev):
            if n != first or 4 * (e - s) < longest[n]:
                continue
            for n2, s2, e2 in ev[i + 1:i + 4] + ev[max(i - 1, 0):i]:      # (before it, where the pair is queued the other way round)
                if n2 in partners:
                    ov = max(0, min(e, e2) - max(s, s2))
                    acc.append((e - s, e2 - s2, ov, max(e, e2) - min(s, s2)))
                    break
        if not acc:
            print("%-58s %5d" % (site, 0))
            continue
        m = [sum(a[k] for a in acc) / len(acc) / 1e6 for k in range(4)]
        short = sum(min(a[0], a[1]) for a in acc)
        print("%-58s %5d %9.3f %9.3f %9.3f %7.1f%% %9.3f %9.3f" % (site, len(acc), m[0], m[1], m[2], 100.0 * sum(a[2] for a in acc) / short,
                                                                    m[3], m[0] + m[1]))


if __name__ == "__main__":
    main(sys.argv[1])
