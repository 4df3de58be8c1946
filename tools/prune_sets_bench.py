"""Measurement for the informed region set between start and goal SETS (gcs_admm_amd/queries.py ``SceneQueries.informed_sets``,
csrc/informed_set_core.h), in the method of tools/prune_bench.py, whose lattices, query classes (``local``, ``corner``) and scipy search
it uses:

  * seconds of ``region_paths`` (the point kernel, whose rounds run until the whole graph has settled) against ``region_paths_sets``
    (the set kernel, whose rounds end under the cheapest goal cost) on the SAME point queries, the boxes degenerate, alternated in one
    process, with ``scipy.sparse.csgraph.dijkstra`` in the same run; every device cost of both calls must agree with scipy's to 1e-12
    relative and the two calls with each other bit for bit, or the run stops;
  * the kept fraction, the path's length and the bound of point -> box and box -> box queries, the box one cell and a block of 3 x 3
    cells (each shrunk by a hundredth of a cell, so that it meets the cells it names and no other), with the seconds of
    ``informed_sets`` as a whole;
  * with ``--solve``: seconds of ``SceneQueries.solve`` for point -> one-cell-box queries with and without ``prune="informed_sets"``,
    alternated after a warm-up of both, with both rounded costs; where the batch refuses a side, the refusal is recorded and the
    other side timed alone.

Medians of ``--repeats`` (default 5) with the spread; every time is a host clock around calls that end in a copy from the device.  One
JSON line per (lattice, class).

  python tools/prune_sets_bench.py [--lattices 20x25 25x40 100x200] [--queries 4] [--solve 20x25 25x40] [--max-it N] [--repeats 5]
"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: F401  (HIP runtime first, see abi.load_library)
from gcs_admm_amd.abi import GcsAdmmError
from gcs_admm_amd.queries import SceneQueries
from prune_bench import clock, host_search, lattice_sets, spread


def query_cells(nx, ny, kind, B, rng):
    """(start cells, goal cells) as (column, row) pairs: the cells of ``prune_bench.query_points``"""
    if kind == "corner":
        return [(k, 0) for k in range(B)], [(nx - 1 - k, ny - 1) for k in range(B)]
    i, j = rng.integers(0, nx - 2, B), rng.integers(0, ny - 3, B)
    return [(int(x), int(y)) for x, y in zip(i, j)], [(int(x) + 2, int(y) + 3) for x, y in zip(i, j)]


def blocks(lo, hi, nx, ny, cells, reach):
    """(lo [B, n], hi [B, n]): per cell the bounding box of the cells within ``reach`` columns and rows of it (0: the cell alone), cut at
    the lattice's rim and shrunk by a hundredth of a cell"""
    out_lo, out_hi = [], []
    for i, j in cells:
        ids = [y * nx + x for x in range(max(i - reach, 0), min(i + reach, nx - 1) + 1) for y in range(max(j - reach, 0), min(j + reach, ny - 1) + 1)]
        inset = 0.01 * (hi[j * nx + i] - lo[j * nx + i])
        out_lo.append(lo[ids].min(axis=0) + inset); out_hi.append(hi[ids].max(axis=0) - inset)
    return np.array(out_lo), np.array(out_hi)


def measure(nx, ny, B, repeats, solve, common):
    As, bs = lattice_sets(nx, ny)
    P = nx * ny
    with SceneQueries(As, bs, 2) as sq:
        lo, hi = sq.scene.regions()[3:5]
        for kind in ("local", "corner"):
            a, b = query_cells(nx, ny, kind, B, np.random.default_rng(P))
            S, G = sq.centers[[j * nx + i for i, j in a]], sq.centers[[j * nx + i for i, j in b]]
            pts = np.vstack([S, G])
            sq.informed_sets(starts=S, goals=G)                         # warm-up; builds the region graph
            regs = sq.regions_at(pts)
            term = sq._term_lists(regs)
            row_ptr, tail, head, _ = sq.scene.region_graph()
            w = np.linalg.norm(sq.centers[tail] - sq.centers[head], axis=1)
            sq.scene.region_paths(pts, *term)                           # (warm-up of the point call)
            t_point, t_sets, t_host = [], [], []
            for _ in range(repeats):
                t0 = clock(); _, cost, status = sq.scene.region_paths(pts, *term); t_point.append(clock() - t0)
                t0 = clock(); paths, cost_s, status_s = sq.scene.region_paths_sets(pts, pts, *term); t_sets.append(clock() - t0)
                dt, d = host_search(sq, row_ptr, head, w, S, regs)
                t_host.append(dt)
                if cost.tobytes() != cost_s.tobytes() or status.tobytes() != status_s.tobytes():
                    raise SystemExit(f"{nx}x{ny} {kind}: the set call differs from the point call on degenerate boxes")
                for i in range(B):
                    want = min(d[i, r] + np.linalg.norm(sq.centers[r] - G[i]) for r in regs[B + i])
                    if status_s[i] != 0 or abs(cost_s[i] - want) > 1e-12 * want:
                        raise SystemExit(f"{nx}x{ny} {kind} query {i}: the device path costs {cost_s[i]}, scipy's {want} (status {status_s[i]})")
            line = {"metric": "informed_region_set_between_sets", "lattice": f"{nx}x{ny}", "regions": P, "region_edges": int(len(tail)), "class": kind,
                    "queries": B, "repeats": repeats, "path_regions": [int(len(p)) for p in paths], "centre_polyline_cost": [float(c) for c in cost_s],
                    "region_paths_s": float(np.median(t_point)), "region_paths_s_spread": spread(t_point),
                    "region_paths_sets_s": float(np.median(t_sets)), "region_paths_sets_s_spread": spread(t_sets),
                    "scipy_dijkstra_s": float(np.median(t_host)), "scipy_dijkstra_s_spread": spread(t_host), "costs_equal_scipy": True,
                    "sets_equal_points_bits": True}
            line["points_over_sets"] = line["region_paths_s"] / line["region_paths_sets_s"]
            for reach, label in ((0, "cell"), (1, "block3x3")):
                gb, sb = blocks(lo, hi, nx, ny, b, reach), blocks(lo, hi, nx, ny, a, reach)
                for name, q in ((f"point_to_{label}", dict(starts=S, goal_boxes=gb)), (f"{label}_to_{label}", dict(start_boxes=sb, goal_boxes=gb))):
                    info = sq.informed_sets(**q)
                    t_all = []
                    for _ in range(repeats):
                        t0 = clock(); sq.informed_sets(**q); t_all.append(clock() - t0)
                    line[name] = {"kept_fraction": [float(r["keep"].mean()) for r in info], "kept_regions": [int(r["keep"].sum()) for r in info],
                                  "path_regions": [int(len(r["path"])) for r in info], "bound": [float(r["bound"]) for r in info],
                                  "informed_sets_s": float(np.median(t_all)), "informed_sets_s_spread": spread(t_all)}
            if solve:
                q = dict(starts=S, goal_boxes=blocks(lo, hi, nx, ny, b, 0))
                sides = {"whole": {}, "pruned": dict(prune="informed_sets")}
                for k, kw in list(sides.items()):                      # warm-up of both; a side the batch refuses is recorded, not timed
                    try:
                        sq.solve(**q, **kw, **common)
                    except GcsAdmmError as e:
                        line[f"solve_{k}_refused"] = str(e)
                        del sides[k]
                t = {k: [] for k in sides}
                for _ in range(repeats):
                    for k, kw in sides.items():
                        t0 = clock(); rec = sq.solve(**q, **kw, **common); t[k].append(clock() - t0)
                        line[f"{k}_rounded_cost"] = [float(r["rounded_cost"]) for r in rec]
                        line[f"{k}_iterations"] = [int(r["iterations"]) for r in rec]
                for k in sides:
                    line[f"solve_{k}_s"] = float(np.median(t[k])); line[f"solve_{k}_s_spread"] = spread(t[k])
                if len(sides) == 2:
                    line["whole_over_pruned"] = line["solve_whole_s"] / line["solve_pruned_s"]
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", nargs="*", default=["20x25", "25x40", "100x200"])
    ap.add_argument("--queries", type=int, default=4)
    ap.add_argument("--solve", nargs="*", default=[], help="the lattices on which solve is timed with and without prune")
    ap.add_argument("--max-it", type=int, default=None, help="max_it of every member of a timed solve (default: the solver's)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    common = {} if args.max_it is None else dict(max_it=args.max_it)
    for name in args.lattices:
        nx, ny = (int(x) for x in name.split("x"))
        measure(nx, ny, args.queries, args.repeats, name in args.solve, common)


if __name__ == "__main__":
    main()
