"""A/B timing of a variant build of the library: python tools/variant_bench.py <path to .so> <workload> [steps] -- the timed window of bench.py on that library.
<workload>: one of bench.py's, or benchmark1 .. benchmark3 (f64, the window after 60 iterations from the zero state; seven windows, their median reported too)."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcs_admm_amd import abi, solver
abi.select_library(sys.argv[1])
import bench
wl = sys.argv[2]; steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
small = wl in ("benchmark1", "benchmark2", "benchmark3")
if small:
    from gcs_admm_amd.cases import load_fixture
    g, dtype = load_fixture(wl)[1], "f64"
else:
    g, dtype, _ = bench.make_workload(wl)
columns = "edge" if g.num_edges >= 20000 else "incidence"
dev = solver.DeviceSolver(g, dtype, device=0, columns=columns)
first = 57 if small else bench.window_start(wl, 3, steps)
rates = sorted(steps / bench.time_window(dev, first, 3, steps) for _ in range(7 if small else 2))
cb = dev.read_control()
out = {"lib": os.path.basename(sys.argv[1]), "workload": wl, "iterations_per_sec": rates[-1], "inner_iters": cb.inner_iters, "inner_failures": cb.inner_failures}
if small:
    out.update(median=rates[len(rates) // 2], min=rates[0], max=rates[-1])
print(json.dumps(out))
