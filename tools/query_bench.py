"""Measurement for many start / goal queries on one scene (gcs_admm_amd/queries.py, locate_kernel in csrc/polytope_lp.hip): seconds per
query graph from ``SceneQueries.graphs`` against a from-scratch ``graph_from_sets_device(..., broad_phase="device")`` on the same sets,
the ``locate`` call alone, and the share of UNDECIDED hits.  Scenes: the generator of tools/bench_overlap.py, P = 1 000 and 20 000 at
n = 2 and one at n = 6; Q = 2 B points for B = 1, 8, 64 queries.  Medians of five, the two sides alternated in every repetition, after a
warm-up of both; every time is a host clock around calls that end in a copy from the device.  A from-scratch build costs the same
whatever B is, so each repetition builds the first ``--scratch`` queries of the line from scratch (default 2) and compares those: the
edge arrays must be equal, or the run stops.  One JSON line per (scene, B).

``--assemble host device`` measures the assembly of the query graphs instead (csrc/query_graph_core.h): seconds per graph of
``SceneQueries.graphs(assemble="device")`` against ``assemble="host"`` on the same object in the same process, the two alternated in
every repetition, medians of five after a warm-up of both, with the spread; every field of every graph must be equal in every
repetition, or the run stops.  Per line also ``DeviceScene.build_region_graph`` alone against ``scene.edge_arrays`` on the same pair
list, the ``query_graphs`` call alone (the kernel, the copies to the host and the cut into views), and the bytes the kernel writes
per query, 4 (8 E + P + 3).  One name alone (``--assemble device``) times that side without a comparison.

  python tools/query_bench.py [--regions 1000 20000] [--regions6 1000] [--batches 1 8 64] [--scratch 2] [--assemble host device]
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: F401  (HIP runtime first, see abi.load_library)
from bench_overlap import scene_polys
from gcs_admm_amd.graph import convert_pt_to_polytope
from gcs_admm_amd.queries import SceneQueries
from gcs_admm_amd.scene import edge_arrays, graph_from_sets_device

ARRAYS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr")
FIELDS = ARRAYS + ("poly_A", "poly_b", "interior")


def from_scratch(As, bs, n, s, t):
    sets_A = {'s': convert_pt_to_polytope(s)[0], 't': convert_pt_to_polytope(t)[0], **As}
    sets_b = {'s': convert_pt_to_polytope(s)[1], 't': convert_pt_to_polytope(t)[1], **bs}
    return graph_from_sets_device(sets_A, sets_b, n, broad_phase="device")


def measure(n, P, batches, scratch, repeats=5):
    rng = np.random.default_rng(n)
    polys = scene_polys(rng, n, P, 3 + n)
    As = {p: A for p, (A, _) in enumerate(polys)}
    bs = {p: b for p, (_, b) in enumerate(polys)}
    t0 = time.perf_counter()
    sq = SceneQueries(As, bs, n)
    t_scene = time.perf_counter() - t0
    with sq:
        for B in batches:
            # starts and goals inside regions: the generator's regions hold a ball of radius 0.5 around their Chebyshev centre
            jitter = np.zeros((2 * B, n)); jitter[:, :2] = rng.uniform(-0.2, 0.2, (2 * B, min(n, 2)))
            pts = sq.centers[rng.integers(0, P, 2 * B)] + jitter
            S, G = pts[:B], pts[B:]
            k = min(B, scratch)
            sq.graphs(S, G); from_scratch(As, bs, n, S[0], G[0])          # warm-up of both sides at this shape
            t_q, t_f, t_l = [], [], []
            for _ in range(repeats):
                t0 = time.perf_counter(); graphs = sq.graphs(S, G); t_q.append((time.perf_counter() - t0) / B)
                last = dict(sq.last)
                t0 = time.perf_counter(); refs = [from_scratch(As, bs, n, S[i], G[i]) for i in range(k)]; t_f.append((time.perf_counter() - t0) / k)
                t0 = time.perf_counter(); sq.scene.locate(pts); t_l.append(time.perf_counter() - t0)
                for g, ref in zip(graphs, refs):
                    if g.keys != ref.keys or not all(np.array_equal(getattr(g, f), getattr(ref, f)) for f in ARRAYS):
                        raise SystemExit(f"n = {n}, P = {P}, B = {B}: a query graph differs from its from-scratch build")
            q, f = float(np.median(t_q)), float(np.median(t_f))
            print(json.dumps({"metric": "seconds_per_query_graph", "n": n, "regions": P, "queries": B, "points": 2 * B,
                              "rows_per_region": int(polys[0][0].shape[0]), "region_edges": int(len(sq.edge_tail)),
                              "queries_s_per_graph": q, "from_scratch_s_per_graph": f, "ratio": f / q,
                              "queries_s_per_graph_spread": [float(min(t_q)), float(max(t_q))],
                              "from_scratch_s_per_graph_spread": [float(min(t_f)), float(max(t_f))],
                              "locate_call_s": float(np.median(t_l)), "hits": last["hits"], "undecided": last["undecided"],
                              "undecided_share": last["undecided"] / max(last["hits"], 1), "from_scratch_builds_compared": k,
                              "scene_setup_s": t_scene, "edges_equal": True}), flush=True)


def same_graphs(got, ref):
    return len(got) == len(ref) and all(
        g.keys == h.keys and (g.n, g.src, g.dst) == (h.n, h.src, h.dst) and all(
            getattr(g, f).dtype == getattr(h, f).dtype and getattr(g, f).shape == getattr(h, f).shape and getattr(g, f).tobytes() == getattr(h, f).tobytes()
            for f in FIELDS) for g, h in zip(got, ref))


def measure_assembly(n, P, batches, sides, repeats=5):
    rng = np.random.default_rng(n)
    polys = scene_polys(rng, n, P, 3 + n)
    As = {p: A for p, (A, _) in enumerate(polys)}
    bs = {p: b for p, (_, b) in enumerate(polys)}
    clock = time.perf_counter
    with SceneQueries(As, bs, n) as sq:
        pairs = sq._pairs
        flags = pairs["flags"] if np.any(pairs["status"] < 0) else None
        for B in batches:
            jitter = np.zeros((2 * B, n)); jitter[:, :2] = rng.uniform(-0.2, 0.2, (2 * B, min(n, 2)))
            pts = sq.centers[rng.integers(0, P, 2 * B)] + jitter
            S, G = pts[:B], pts[B:]
            for side in sides:                                   # warm-up of every side at this shape
                sq.graphs(S, G, assemble=side)
            regs = sq.regions_at(pts)
            term_ptr = np.zeros(2 * B + 1, np.int64); term_ptr[1:] = np.cumsum([len(r) for r in regs])
            term_region = np.concatenate(regs)
            st = np.array([np.all(np.abs(S[i] - G[i]) <= 2e-6 + 1e-9) for i in range(B)], np.uint8)
            t = {side: [] for side in sides}
            t_build, t_edges, t_call = [], [], []
            for _ in range(repeats):
                graphs = {}
                for side in sides:
                    t0 = clock(); graphs[side] = sq.graphs(S, G, assemble=side); t[side].append((clock() - t0) / B)
                if len(sides) == 2 and not same_graphs(graphs["device"], graphs["host"]):
                    raise SystemExit(f"n = {n}, P = {P}, B = {B}: a device-assembled query graph differs from the host path's")
                t0 = clock(); tail, head = edge_arrays(pairs["pa"], pairs["pb"], pairs["flags"]); t_edges.append(clock() - t0)
                if "device" in sides:
                    t0 = clock(); sq.scene.build_region_graph(flags); t_build.append(clock() - t0)
                    _, dt, dh, _ = sq.scene.region_graph()
                    if not (np.array_equal(dt, tail) and np.array_equal(dh, head)):
                        raise SystemExit(f"n = {n}, P = {P}: the device region graph differs from edge_arrays")
                    t0 = clock(); sq.scene.query_graphs(term_ptr, term_region, st); t_call.append(clock() - t0)
            E = [int(len(g.edge_tail)) for g in graphs[sides[-1]]]
            line = {"metric": "seconds_per_query_graph_by_assembly", "n": n, "regions": P, "queries": B, "rows_per_region": int(polys[0][0].shape[0]),
                    "region_edges": int(len(sq.edge_tail)), "edges_per_graph_mean": float(np.mean(E)),
                    "kernel_bytes_written": int(sum(4 * (8 * e + P + 3) for e in E)), "repeats": repeats,
                    "edge_arrays_s": float(np.median(t_edges)), "edge_arrays_s_spread": [float(min(t_edges)), float(max(t_edges))]}
            for side in sides:
                line[f"{side}_s_per_graph"] = float(np.median(t[side]))
                line[f"{side}_s_per_graph_spread"] = [float(min(t[side])), float(max(t[side]))]
            if "device" in sides:
                line.update(build_region_graph_s=float(np.median(t_build)), build_region_graph_s_spread=[float(min(t_build)), float(max(t_build))],
                            query_graphs_call_s=float(np.median(t_call)), query_graphs_call_s_spread=[float(min(t_call)), float(max(t_call))])
            if len(sides) == 2:
                line.update(host_over_device=line["host_s_per_graph"] / line["device_s_per_graph"], arrays_equal=True)
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, nargs="*", default=[1000, 20000])
    ap.add_argument("--regions6", type=int, default=1000)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--scratch", type=int, default=2)
    ap.add_argument("--assemble", nargs="*", choices=["host", "device"], default=None,
                    help="measure the assembly of the query graphs on these sides (both: alternated and compared) instead of the from-scratch lines")
    args = ap.parse_args()
    if args.assemble:
        sides = [s for s in ("host", "device") if s in args.assemble]
        run = lambda n, P: measure_assembly(n, P, args.batches, sides)
    else:
        run = lambda n, P: measure(n, P, args.batches, args.scratch)
    for P in args.regions:
        run(2, P)
    if args.regions6:
        run(6, args.regions6)


if __name__ == "__main__":
    main()
