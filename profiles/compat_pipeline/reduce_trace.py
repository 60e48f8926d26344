"""rocprofv3 --kernel-trace output directory -> the dispatches in dispatch order, the runtime's fill and copy kernels included, as text:
first a legend, one line per distinct (kernel, grid, workgroup, LDS) numbered in order of first appearance, then an empty line, then the
legend numbers of all dispatches in order, 40 to a line.  Two traces make the same launches exactly when the two files are byte-identical.
Usage: python reduce_trace.py <trace dir> <out.txt>"""
import csv
import glob
import sys

rows = []
for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)):
    rows += list(csv.DictReader(open(f)))
assert rows, "no kernel trace under " + sys.argv[1]
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
legend, order = {}, []
for r in rows:
    key = (r["Kernel_Name"], "x".join(r["Grid_Size_" + a] for a in "XYZ"), "x".join(r["Workgroup_Size_" + a] for a in "XYZ"), r["LDS_Block_Size"])
    order.append(legend.setdefault(key, len(legend)))
with open(sys.argv[2], "w", newline="") as out:
    w = csv.writer(out, lineterminator="\n")
    w.writerow(["id", "kernel", "grid", "workgroup", "lds"])
    for key, i in legend.items():
        w.writerow([i, *key])
    out.write("\n")
    for at in range(0, len(order), 40):
        out.write(" ".join(map(str, order[at: at + 40])) + "\n")
print(len(rows), "dispatches,", len(legend), "distinct ->", sys.argv[2])
