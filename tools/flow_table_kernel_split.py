"""Per-kernel split of the flow table's update from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -o a --output-format csv -- \\
        python tools/flow_table_bench.py --configs c3 --rows a --runs 1
    (the same with --rows b and -o b)
    python tools/flow_table_kernel_split.py OUT.csv a=DIR/.../a_kernel_trace.csv b=DIR/.../b_kernel_trace.csv

tools/flow_table_bench.py calls the same kernels in its warm-up and in both
rows, so the trace's own per-name statistics mix them. This keeps, per kernel
name, the last --last dispatches of a trace: the timed repetitions of the row
that ran last.
"""
import argparse
import collections
import csv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("traces", nargs="+", help="row=kernel_trace.csv")
    ap.add_argument("--last", type=int, default=5)
    a = ap.parse_args()
    with open(a.out, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Row", "Name", "Calls", "AverageNs", "MinNs", "MaxNs"])
        for spec in a.traces:
            row, path = spec.split("=", 1)
            calls = collections.defaultdict(list)
            for r in csv.DictReader(open(path)):
                if "zp_flow" in r["Kernel_Name"]:
                    calls[r["Kernel_Name"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
            for name, v in sorted(calls.items(), key=lambda kv: max(s for s, _ in kv[1])):
                d = [e - s for s, e in sorted(v)[-a.last:]]
                w.writerow([row, name.split("(")[0], len(d), sum(d) / len(d), min(d), max(d)])


if __name__ == "__main__":
    main()
