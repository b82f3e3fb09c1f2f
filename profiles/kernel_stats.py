"""Per-kernel launches and time of the timed region of a traced bench run, the table of profiles/r08_kernel_stats_*.txt and
r09_kernel_stats_*.txt.  Usage:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --steps 20
    python profiles/kernel_stats.py DIR MS_PER_STEP [STEPS]

DIR is searched for *kernel_trace.csv (the largest one: the bench process); MS_PER_STEP is what that run printed.  Rows: kernels
whose dispatch starts in the last STEPS x MS_PER_STEP of the trace (= the timed region: STEPS complete batches), summed kernel
durations (launches of different lanes overlap)."""
import collections
import csv
import glob
import os
import sys


def short(n):
    n = n.replace("(anonymous namespace)::", "").replace("void ", "")
    return n.split("(")[0].split("<")[0][:56]


def main(root, ms_per_step, steps=20):
    paths = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit("no *kernel_trace.csv under %s" % root)
    path = max(paths, key=os.path.getsize)
    rows = list(csv.DictReader(open(path)))
    end = max(int(r["End_Timestamp"]) for r in rows)
    t0 = end - steps * ms_per_step * 1e6
    agg = collections.defaultdict(lambda: [0, 0])
    for r in rows:
        if int(r["Start_Timestamp"]) >= t0:
            a = agg[short(r["Kernel_Name"])]
            a[0] += 1
            a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    print("%-58s %10s %12s %12s %14s" % ("kernel", "launches", "total ms", "ms per step", "us per launch"))
    for name, (n, ns) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print("%-58s %10d %12.2f %12.3f %14.1f" % (name, n, ns / 1e6, ns / 1e6 / steps, ns / 1e3 / n))
    n_all, ns_all = sum(v[0] for v in agg.values()), sum(v[1] for v in agg.values())
    print("%-58s %10d %12.2f %12.3f" % ("ALL KERNELS", n_all, ns_all / 1e6, ns_all / 1e6 / steps))


if __name__ == "__main__":
    main(sys.argv[1], float(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 20)
