"""rocprofv3 --kernel-trace CSV of `tools/time_eval_forward.py --trace B --iters N` -> launches and kernel time per forward.

    python tools/eval_forward_trace.py TRACE_DIR N

The dispatches after the largest gap between two consecutive kernels (the tool's 2 s pause behind its warm-up forward) are
the N measured forwards.  Prints the per-forward totals, then every kernel: launches and microseconds per forward."""
import collections
import csv
import glob
import sys


def per_forward(trace_dir, n):
    """{kernel name: (launches, us)} per forward."""
    path = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    starts = [int(r["Start_Timestamp"]) for r in rows]
    cut = max(range(1, len(rows)), key=lambda i: starts[i] - int(rows[i - 1]["End_Timestamp"]))
    agg = collections.defaultdict(list)
    for r in rows[cut:]:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")[:80]
        agg[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (len(v) / n, sum(v) / n) for k, v in agg.items()}


def main():
    kernels = per_forward(sys.argv[1], int(sys.argv[2]))
    print("per forward: %.1f launches, %.1f us of kernel time" % (sum(c for c, _ in kernels.values()),
                                                                  sum(t for _, t in kernels.values())))
    for name, (count, us) in sorted(kernels.items(), key=lambda kv: -kv[1][1]):
        print("  %6.1f x  %8.2f us  %s" % (count, us, name))


if __name__ == "__main__":
    main()
