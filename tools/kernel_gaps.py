"""Development probe: idle time between consecutive kernels of the loop, from a rocprofv3 --kernel-trace csv
(rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --full --loop-only ...; python3 tools/kernel_gaps.py DIR)."""
import csv, glob, sys
import numpy as np
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
st = np.array([int(r["Start_Timestamp"]) for r in rows]); en = np.array([int(r["End_Timestamp"]) for r in rows])
names = [r["Kernel_Name"] for r in rows]
kind = np.array([0 if "vertex" in n else (1 if "edge_kernel" in n else 2) for n in names])
gap = st[1:] - en[:-1]
tail = slice(len(rows) // 2, None)          # the second half: the timed window, not the set-up
for a, b, label in ((0, 1, "vertex -> edge"), (1, 0, "edge -> vertex")):
    m = (kind[:-1] == a) & (kind[1:] == b)
    m[:len(rows) // 2] = False
    print(f"{label}: {m.sum()} gaps, mean {gap[m].mean() / 1e3:.2f} us, median {np.median(gap[m]) / 1e3:.2f} us")
for k, label in ((0, "vertex kernel"), (1, "edge kernel")):
    m = kind == k; m[:len(rows) // 2] = False
    print(f"{label}: mean {(en - st)[m].mean() / 1e3:.2f} us")
v = np.nonzero((kind == 0))[0]; v = v[v >= len(rows) // 2]
print(f"vertex start to vertex start: mean {np.diff(st[v]).mean() / 1e3:.2f} us")
