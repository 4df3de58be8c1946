"""Measurement for the informed region set of a query (gcs_admm_amd/queries.py ``SceneQueries.informed``, csrc/informed_core.h): on brick
lattices of ``graph.lattice_boxes`` (default 25x40 = 1 000 and 100x200 = 20 000 regions), for two classes of queries -- ``local`` (the
goal a few cells from the start) and ``corner`` (first cell to last cell) --

  * the kept fraction per query, with the candidate path's length, its centre-polyline cost and the bound;
  * seconds of the two scene calls (``region_paths``: kernel, copies, the cut into paths; ``informed_regions``) and of ``informed`` as a
    whole (locate, both calls and the device restriction), against ``scipy.sparse.csgraph.dijkstra`` on the same graph with the same
    weights from the same start regions in the same run; the two costs must agree to 1e-12 relative, or the run stops;
  * with ``--solve``: seconds of ``SceneQueries.solve`` with and without ``prune="informed"``, alternated in one process on the same
    queries after a warm-up of both, with both rounded costs per query.  "Without" is the code path of a solve that knows no pruning;
    where the batch refuses a side (a member of 512 vertices or more), the refusal is recorded and the other side timed alone.
  * with ``--assemble``: seconds of the assembly of the pruned graphs alone, on the keep flags ``informed`` returned: the host's
    (``_host_graph(keep)``: a mask over all region edges, a ``lexsort`` and ``graph._finish_graph`` per query) against the device's
    (``assemble="induced"``: one ``induced_query_graphs`` call, csrc/induced_graph_core.h, and the gather of the kept polytope rows),
    alternated in one process on the same queries after a warm-up of both, and the ``induced_sizes`` call alone; the graphs of the two
    must be equal byte for byte, or the run stops.

Medians of ``--repeats`` (default 5) with the spread; every time is a host clock around calls that end in a copy from the device.  One
JSON line per (lattice, class).

  python tools/prune_bench.py [--lattices 25x40 100x200] [--queries 4] [--solve 25x40] [--assemble] [--max-it N] [--repeats 5]
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401  (HIP runtime first, see abi.load_library)
from gcs_admm_amd.abi import GcsAdmmError
from gcs_admm_amd.graph import lattice_boxes
from gcs_admm_amd.queries import SceneQueries

clock = time.perf_counter


def lattice_sets(nx, ny):
    g = lattice_boxes(nx, ny)
    cells = range(2, g.num_vertices)
    return ({("cell", v - 2): g.poly_A[g.poly_ptr[v]:g.poly_ptr[v + 1]] for v in cells},
            {("cell", v - 2): g.poly_b[g.poly_ptr[v]:g.poly_ptr[v + 1]] for v in cells})


def query_points(sq, nx, ny, kind, B, rng):
    """starts and goals at the centres of cells: ``local`` from a random cell to the one 2 columns and 3 rows on, ``corner`` from the
    first cells of the first row to the last cells of the last row"""
    cell = lambda i, j: j * nx + i
    if kind == "corner":
        a = [cell(k, 0) for k in range(B)]; b = [cell(nx - 1 - k, ny - 1) for k in range(B)]
    else:
        i, j = rng.integers(0, nx - 2, B), rng.integers(0, ny - 3, B)
        a = [cell(x, y) for x, y in zip(i, j)]; b = [cell(x + 2, y + 3) for x, y in zip(i, j)]
    return sq.centers[a], sq.centers[b]


def spread(t):
    return [float(min(t)), float(max(t))]


def host_search(sq, row_ptr, head, w, S, regs):
    """scipy's Dijkstra from the start regions of every query through one extra source vertex per query: (seconds, distances [B, P])"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    P, B = len(row_ptr) - 1, len(S)
    t0 = clock()
    out = np.empty((B, P))
    for i in range(B):      # the source's edges differ per query: one matrix per query, as a host search would build it
        rs = regs[i]
        init = np.linalg.norm(sq.centers[rs] - S[i], axis=1)
        indptr = np.concatenate([row_ptr, [row_ptr[-1] + len(rs)]])
        # a weight of exactly 0 would be dropped as "no edge": the start's own region lies at distance > 0 unless the point is its centre
        m = csr_matrix((np.concatenate([w, np.maximum(init, 1e-300)]), np.concatenate([head, rs]), indptr), shape=(P + 1, P + 1))
        out[i] = dijkstra(m, directed=True, indices=P)[:P]
    return clock() - t0, out


GRAPH_FIELDS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr", "poly_A", "poly_b", "interior")


def time_assembly(sq, S, G, regs, info, repeats, eps=1e-6):
    """the fields of a line for ``--assemble``: host-pruned against induced assembly of the same graphs, alternated"""
    B = len(S)
    sides = {"host": lambda: [sq._host_graph(S[i], G[i], regs[i], regs[B + i], eps, info[i]["keep"]) for i in range(B)],
             "induced": lambda: sq._assemble_induced(S, G, regs, eps, info)}
    first = {k: f() for k, f in sides.items()}                         # warm-up of both
    for g, h in zip(first["host"], first["induced"]):
        if g.keys != h.keys or any(getattr(g, f).dtype != getattr(h, f).dtype or getattr(g, f).tobytes() != getattr(h, f).tobytes() for f in GRAPH_FIELDS):
            raise SystemExit("the induced assembly differs from the host-pruned graphs")
    keep = np.array([r["keep"] for r in info], np.uint8)
    term = sq._term_lists(regs)
    st = sq._adjacent(S, G, eps)
    t = {k: [] for k in sides}
    t_sizes = []
    for _ in range(repeats):
        for k, f in sides.items():
            t0 = clock(); f(); t[k].append(clock() - t0)
        t0 = clock(); sq.scene.induced_sizes(keep, *term, st); t_sizes.append(clock() - t0)
    out = {"graph_vertices": [int(g.num_vertices) for g in first["host"]], "graph_edges": [int(len(g.edge_tail)) for g in first["host"]],
           "graphs_equal": True, "induced_sizes_s": float(np.median(t_sizes)), "induced_sizes_s_spread": spread(t_sizes)}
    for k in sides:
        out[f"assemble_{k}_s"] = float(np.median(t[k])); out[f"assemble_{k}_s_spread"] = spread(t[k])
    out["host_over_induced"] = out["assemble_host_s"] / out["assemble_induced_s"]
    return out


def measure(nx, ny, B, repeats, solve, common, assemble=False):
    As, bs = lattice_sets(nx, ny)
    P = nx * ny
    rng = np.random.default_rng(P)
    with SceneQueries(As, bs, 2) as sq:
        for kind in ("local", "corner"):
            S, G = query_points(sq, nx, ny, kind, B, rng)
            pts = np.vstack([S, G])
            info = sq.informed(S, G)                                   # warm-up; builds the region graph
            regs = sq.regions_at(pts)
            term = sq._term_lists(regs)
            row_ptr, tail, head, _ = sq.scene.region_graph()
            w = np.linalg.norm(sq.centers[tail] - sq.centers[head], axis=1)
            bound = np.array([r["bound"] for r in info])
            t_paths, t_keep, t_all, t_host = [], [], [], []
            for _ in range(repeats):
                t0 = clock(); paths, cost, status = sq.scene.region_paths(pts, *term); t_paths.append(clock() - t0)
                t0 = clock(); sq.scene.informed_regions(pts, bound); t_keep.append(clock() - t0)
                t0 = clock(); sq.informed(S, G); t_all.append(clock() - t0)
                dt, d = host_search(sq, row_ptr, head, w, S, regs)
                t_host.append(dt)
                for i in range(B):
                    want = min(d[i, r] + np.linalg.norm(sq.centers[r] - G[i]) for r in regs[B + i])
                    if status[i] != 0 or abs(cost[i] - want) > 1e-12 * want:
                        raise SystemExit(f"{nx}x{ny} {kind} query {i}: the device path costs {cost[i]}, scipy's {want} (status {status[i]})")
            line = {"metric": "informed_region_set", "lattice": f"{nx}x{ny}", "regions": P, "region_edges": int(len(tail)), "class": kind, "queries": B,
                    "repeats": repeats, "kept_fraction": [float(r["keep"].mean()) for r in info], "kept_regions": [int(r["keep"].sum()) for r in info],
                    "path_regions": [int(len(r["path"])) for r in info], "centre_polyline_cost": [float(c) for c in cost],
                    "bound": [float(b) for b in bound],
                    "region_paths_s": float(np.median(t_paths)), "region_paths_s_spread": spread(t_paths),
                    "informed_regions_s": float(np.median(t_keep)), "informed_regions_s_spread": spread(t_keep),
                    "informed_s": float(np.median(t_all)), "informed_s_spread": spread(t_all),
                    "scipy_dijkstra_s": float(np.median(t_host)), "scipy_dijkstra_s_spread": spread(t_host), "costs_equal_scipy": True}
            if assemble:
                line.update(time_assembly(sq, S, G, regs, info, repeats))
            if solve:
                sides = {"whole": {}, "pruned": dict(prune="informed")}
                for k, kw in list(sides.items()):                      # warm-up of both; a side the batch refuses is recorded, not timed
                    try:
                        sq.solve(S, G, **kw, **common)
                    except GcsAdmmError as e:
                        line[f"solve_{k}_refused"] = str(e)
                        del sides[k]
                t = {k: [] for k in sides}
                for _ in range(repeats):
                    for k, kw in sides.items():
                        t0 = clock(); rec = sq.solve(S, G, **kw, **common); t[k].append(clock() - t0)
                        line[f"{k}_rounded_cost"] = [float(r["rounded_cost"]) for r in rec]
                        line[f"{k}_iterations"] = [int(r["iterations"]) for r in rec]
                for k in sides:
                    line[f"solve_{k}_s"] = float(np.median(t[k])); line[f"solve_{k}_s_spread"] = spread(t[k])
                if len(sides) == 2:
                    line["whole_over_pruned"] = line["solve_whole_s"] / line["solve_pruned_s"]
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", nargs="*", default=["25x40", "100x200"])
    ap.add_argument("--queries", type=int, default=4)
    ap.add_argument("--solve", nargs="*", default=[], help="the lattices on which solve is timed with and without prune")
    ap.add_argument("--assemble", action="store_true", help="time the host-pruned against the induced assembly of the pruned graphs")
    ap.add_argument("--max-it", type=int, default=None, help="max_it of every member of a timed solve (default: the solver's)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    common = {} if args.max_it is None else dict(max_it=args.max_it)
    for name in args.lattices:
        nx, ny = (int(x) for x in name.split("x"))
        measure(nx, ny, args.queries, args.repeats, name in args.solve, common, args.assemble)


if __name__ == "__main__":
    main()
