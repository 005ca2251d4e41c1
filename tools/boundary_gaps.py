#!/usr/bin/env python3
"""Where one LM iteration's time goes, from a rocprofv3 kernel trace: for the five-launch cycle of the speculative
chain (k_schur, k_S_reduce, k_chol_tiles, k_update_lin, k_cam_reduce) the median duration of each kernel and the
median gap from its end to the start of the next dispatch.  A launch that leaves dirty lines in the L2s shows up in
its own gap (the write-back at the kernel boundary), not in its duration.

    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python3 bench.py --only C2 --steps 20 --warmup 5
    tools/boundary_gaps.py DIR/.../run_kernel_trace.csv [--skip CYCLES] [--label TEXT]

Pure Python, no GPU.  Timestamps are nanoseconds; the table is in microseconds."""
import argparse
import csv
import re
import statistics

CYCLE = ("k_schur", "k_S_reduce", "k_chol_tiles", "k_update_lin", "k_cam_reduce")


def short_name(name):
    """'void sg::k_update_lin<false, 2>(sg::Dev)' -> 'k_update_lin'."""
    m = re.search(r"(k_[A-Za-z0-9_]+)", name)
    return m.group(1) if m else name


def read_trace(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short_name(r["Kernel_Name"])))
    rows.sort()
    return rows


def cycles(rows):
    """Index of every dispatch that starts a complete cycle followed by one more dispatch."""
    n = len(CYCLE)
    out, i = [], 0
    while i + n < len(rows):
        if all(rows[i + k][2] == CYCLE[k] for k in range(n)):
            out.append(i)
            i += n
        else:
            i += 1
    return out


def table(rows, skip=0):
    starts = cycles(rows)[skip:]
    dur = {k: [] for k in CYCLE}
    gap = {k: [] for k in CYCLE}
    span = []
    for i in starts:
        for k, name in enumerate(CYCLE):
            s, e, _ = rows[i + k]
            dur[name].append((e - s) * 1e-3)
            gap[name].append((rows[i + k + 1][0] - e) * 1e-3)
        span.append((rows[i + len(CYCLE)][0] - rows[i][0]) * 1e-3)
    return starts, dur, gap, span


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("csv")
    ap.add_argument("--skip", type=int, default=5, help="leading cycles left out (warm-up)")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    rows = read_trace(a.csv)
    starts, dur, gap, span = table(rows, a.skip)
    if not starts:
        raise SystemExit("no complete %s cycle in %s" % (" > ".join(CYCLE), a.csv))
    print("%s%d cycles (after %d skipped), medians in us" % (a.label + ": " if a.label else "", len(starts), a.skip))
    print("%-14s %9s %9s %9s" % ("kernel", "duration", "gap after", "sum"))
    td = tg = 0.0
    for k in CYCLE:
        d, g = statistics.median(dur[k]), statistics.median(gap[k])
        td += d
        tg += g
        print("%-14s %9.2f %9.2f %9.2f" % (k, d, g, d + g))
    print("%-14s %9.2f %9.2f %9.2f" % ("sum of medians", td, tg, td + tg))
    print("%-14s %29.2f" % ("median cycle", statistics.median(span)))


if __name__ == "__main__":
    main()
