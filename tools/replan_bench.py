"""Measurement for replanning (gcs_admm_amd/transfer.py; csrc/state_transfer_core.h): a start that moves in K steps along a line, on
benchmark4's regions and on a box lattice scene; every step is solved cold (from zero: ``SceneQueries.solve`` as it was before seeds
existed, the same code path) and solved seeded from the snapshot of the step before, alternated in one process after a warm-up of
both.

Per step: the iterations of each, the rounded costs, seconds of the whole ``solve`` call (locate, graph, batch, loop, rounding) and of
the loop alone (the records' ``wall_time_s``; the seeded one includes its import).  Per scene: seconds of one
``BatchSolver.import_state`` and one ``export_state`` call alone on the last step's graph (host clock around a call that ends in a
stream synchronise), next to the member's seconds per ADMM iteration (cold loop seconds / cold iterations): the two calls pay for
themselves when they cost less than the iterations a seed saves.  Medians of ``--repeats`` with the spread.  One JSON line per scene.

  python tools/replan_bench.py [--steps 8] [--step 0.05] [--lattice 12x12] [--repeats 5] [--prune]
"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: F401  (HIP runtime first, see abi.load_library)
from gcs_admm_amd import BatchSolver
from gcs_admm_amd.cases import fixture_sets, load_fixture
from gcs_admm_amd.queries import SceneQueries
from prune_bench import clock, lattice_sets, spread


def scenes(lattice):
    """(name, As, bs, n, first start, goal, unit direction of the start's motion)"""
    As, bs, n, _, _ = fixture_sets("benchmark4")
    g = load_fixture("benchmark4")[1]
    yield ("benchmark4", {k: As[k] for k in As if k not in ('s', 't')}, {k: bs[k] for k in bs if k not in ('s', 't')}, n,
           g.interior[g.src].copy(), g.interior[g.dst].copy(), np.array([1.0, 0.0]))
    nx, ny = (int(x) for x in lattice.split("x"))
    As, bs = lattice_sets(nx, ny)
    box = lambda k: (-bs[("cell", k)][2:], bs[("cell", k)][:2])      # rows [I; -I] x <= [hi; -lo]
    (lo0, hi0), (lo1, hi1) = box(0), box(nx * ny - 1)
    yield (f"lattice{lattice}", As, bs, 2, 0.5 * (lo0 + hi0) - np.array([0.3 * (hi0[0] - lo0[0]), 0.0]), 0.5 * (lo1 + hi1), np.array([1.0, 0.0]))


def measure(name, As, bs, n, s0, goal, direction, steps, step, repeats, how):
    med = lambda t: float(np.median(t))
    with SceneQueries(As, bs, n) as sq:
        G = goal[None]
        start = lambda k: (s0 + k * step * direction)[None]
        sq.solve(start(0), G, **how)                                   # warm-up of the cold path
        prev, = sq.solve(start(0), G, keep=True, **how)
        warm, = sq.solve(start(0), G, seed=[prev["snapshot"]], keep=True, **how)      # ... and of the seeded one
        warm["snapshot"].close()
        rows = []
        for k in range(1, steps + 1):
            S = start(k)
            t = dict(cold=[], seeded=[]); loop = dict(cold=[], seeded=[])
            for rep in range(repeats):
                t0 = clock(); cold, = sq.solve(S, G, **how); t["cold"].append(clock() - t0); loop["cold"].append(cold["wall_time_s"])
                t0 = clock(); seeded, = sq.solve(S, G, seed=[prev["snapshot"]], keep=True, **how); t["seeded"].append(clock() - t0)
                loop["seeded"].append(seeded["wall_time_s"])
                if rep < repeats - 1:
                    seeded["snapshot"].close()
            rows.append(dict(step=k, cold_iterations=int(cold["iterations"]), seeded_iterations=int(seeded["iterations"]),
                             cold_rounded_cost=float(cold["rounded_cost"]), seeded_rounded_cost=float(seeded["rounded_cost"]),
                             cold_solve_s=med(t["cold"]), cold_solve_s_spread=spread(t["cold"]), seeded_solve_s=med(t["seeded"]),
                             seeded_solve_s_spread=spread(t["seeded"]), cold_loop_s=med(loop["cold"]), seeded_loop_s=med(loop["seeded"]),
                             vertices=int(cold["graph"].num_vertices), edges=int(cold["graph"].num_edges)))
            prev["snapshot"].close()
            prev = seeded
        # the two calls alone, on the last step's graph
        g = prev["graph"]
        ids = [sq.vertex_ids(g)]
        batch = BatchSolver([g], "f64", device=sq.device)
        batch.reset()
        batch.import_state([prev["snapshot"]], ids); batch.export_state(ids)[0].close()      # warm-up
        t_imp, t_exp = [], []
        for _ in range(max(repeats, 5)):
            torch.cuda.synchronize()
            t0 = clock(); batch.import_state([prev["snapshot"]], ids); t_imp.append(clock() - t0)
            t0 = clock(); snap = batch.export_state(ids); t_exp.append(clock() - t0)
            snap[0].close()
        batch.close()
        for m in batch.members:
            m.close()
        prev["snapshot"].close()
    per_it = float(np.median([r["cold_loop_s"] / r["cold_iterations"] for r in rows]))
    line = dict(metric="replanning_seeded_from_the_step_before", scene=name, regions=len(As), steps=steps, step=step, repeats=repeats, how=how,
                rows=rows, import_call_s=med(t_imp), import_call_s_spread=spread(t_imp), export_call_s=med(t_exp), export_call_s_spread=spread(t_exp),
                cold_loop_s_per_iteration=per_it, import_plus_export_in_iterations=(med(t_imp) + med(t_exp)) / per_it,
                iterations_saved_median=float(np.median([r["cold_iterations"] - r["seeded_iterations"] for r in rows])),
                costs_agree_1e5=bool(all(abs(r["cold_rounded_cost"] - r["seeded_rounded_cost"]) <= 1e-5 for r in rows)))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--step", type=float, default=0.05)
    ap.add_argument("--lattice", default="12x12")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--prune", action="store_true", help='prune="informed", assemble="induced"')
    args = ap.parse_args()
    how = dict(prune="informed", assemble="induced") if args.prune else {}
    for scene in scenes(args.lattice):
        measure(*scene, args.steps, args.step, args.repeats, how)


if __name__ == "__main__":
    main()
