"""Throughput of queries with a start point and a goal BOX, as one batch against solo handles one after another.

    python tools/terminal_batch_bench.py [--sizes 1,2,4,8,16,32] [--lattice 6] [--iters 200] [--reps 5] [--out profiles/batch_terminals/result.json]

B queries on an L x L lattice scene (graph.lattice_boxes), each from a point near a cell's centre to a box of half-widths 0.1 .. 0.45
about another cell's centre, so every query graph has a terminal that is a region.  Each problem gets its own rho in [0.5, 2] and the
stop test is switched off (eps_abs = eps_rel = 0), so every run is exactly ``--iters`` iterations of every problem.  Two ways to do
that work, alternated inside every repetition:
  batch   one BatchSolver(region_terminals=True): per iteration one vertex launch, one terminal launch per group of terminals and one
          edge + control launch for all B problems
  solo    the same B problems one after another, each on its own DeviceSolver(program="workgroup256") -- all that can be done
          without GCSADMM_BATCH_TERMINALS, since a batch refuses such a member: the baseline
The rate is aggregate problem-iterations per second of wall time around work that ends in a device synchronise; medians of the
repetitions after one warm-up, with the spread (min .. max), as tools/batch_bench.py reports them.

Also timed, for the boxes of the largest B (median and spread of ``--reps`` runs): one ``DeviceScene.locate_boxes`` call (with the
read-back of the hit list) against the host decisions ``graph_from_sets`` makes for the same terminals -- ``graph.polytopes_overlap``
of every box with every region.  Needs the GPU; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def queries(L, B, seed=6):
    """(As, bs of the L x L cells, start points [B, 2], (lo, hi) of the goal boxes)"""
    import numpy as np
    from gcs_admm_amd.graph import lattice_boxes, sets_of_graph
    As, bs = sets_of_graph(lattice_boxes(L, L))
    As = {k: np.array(v) for k, v in As.items() if k not in ('s', 't')}; bs = {k: np.array(v) for k, v in bs.items() if k not in ('s', 't')}
    cen = np.array([0.5 * (bs[k][:2] - bs[k][2:]) for k in As])
    rng = np.random.default_rng(seed)
    S = cen[rng.integers(0, len(cen), B)] + rng.uniform(-0.1, 0.1, (B, 2))
    c, h = cen[rng.integers(0, len(cen), B)], rng.uniform(0.1, 0.45, (B, 2))
    return As, bs, S, (c - h, c + h)


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--lattice", type=int, default=6)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gcs_admm_amd import BatchSolver, SceneQueries
    from gcs_admm_amd.graph import polytopes_overlap
    from gcs_admm_amd.solver import DeviceSolver
    assert torch.cuda.is_available(), "terminal_batch_bench needs a GPU"
    K = args.iters
    fixed = dict(eps_abs=0.0, eps_rel=0.0, max_it=K + 1)
    sync = lambda: torch.cuda.synchronize(0)
    sizes = [int(s) for s in args.sizes.split(",")]
    As, bs, S, gb = queries(args.lattice, max(sizes))
    with SceneQueries(As, bs, 2) as sq:
        all_graphs = sq.graphs(starts=S, goal_boxes=gb)
        # one locate_boxes call against the host's decisions for the same boxes
        t_dev, t_host = [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter(); hits = sq.scene.locate_boxes(*gb); dt = time.perf_counter() - t0
            if rep > 0:
                t_dev.append(dt)
        box = lambda q: (np.vstack([np.eye(2), -np.eye(2)]), np.hstack([gb[1][q], -gb[0][q]]))
        for rep in range(args.reps):
            t0 = time.perf_counter()
            met = sum(polytopes_overlap(*box(q), *poly) for q in range(len(S)) for poly in sq.polys)
            t_host.append(time.perf_counter() - t0)
        locate = dict(boxes=len(S), regions=len(sq.polys), hits=int(len(hits[1])), undecided=int((hits[2] == 2).sum()), overlapping_pairs=int(met),
                      locate_boxes_ms={k: 1e3 * v for k, v in spread(t_dev).items()}, host_decisions_ms={k: 1e3 * v for k, v in spread(t_host).items()})
    print(f"locate_boxes {locate['locate_boxes_ms']['median']:.3f} ms   host decisions {locate['host_decisions_ms']['median']:.3f} ms   "
          f"({locate['boxes']} boxes x {locate['regions']} regions, {locate['hits']} hits, {locate['undecided']} undecided)", file=sys.stderr, flush=True)
    rows = []
    for B in sizes:
        graphs = all_graphs[:B]
        params = [dict(rho=r) for r in ([1.0] if B == 1 else [float(r) for r in np.linspace(0.5, 2.0, B)])]
        batch = BatchSolver(graphs, "f64", device=0, region_terminals=True)
        solos = [DeviceSolver(g, "f64", device=0, program="workgroup256") for g in graphs]

        def run_batch():
            batch.reset(params, **fixed)
            sync(); t0 = time.perf_counter()
            batch.enqueue(K)
            status, it = batch.poll()
            dt = time.perf_counter() - t0
            assert all(i == K + 1 for i in it), it
            return dt

        def run_solos():
            for d, p in zip(solos, params):
                d.reset(**p, **fixed)
            sync(); t0 = time.perf_counter()
            for d in solos:
                d.enqueue(K)
                assert d.read_control().it == K + 1
            return time.perf_counter() - t0

        ways = dict(batch=run_batch, solo=run_solos)
        times = {k: [] for k in ways}
        for rep in range(args.reps + 1):
            for k, f in ways.items():
                dt = f()
                if rep > 0:       # the first round warms up every shape
                    times[k].append(dt)
        row = dict(B=B, iters=K, reps=args.reps, vertices=int(graphs[0].num_vertices), terminal_launches=batch.terminal_launches())
        for k, dts in times.items():
            row[k] = spread([B * K / dt for dt in dts])
        row["speedup"] = row["batch"]["median"] / row["solo"]["median"]
        rows.append(row)
        print(f"B={B:3d}  batch {row['batch']['median']:10.0f} it/s ({row['batch']['min']:.0f} .. {row['batch']['max']:.0f})   "
              f"solo {row['solo']['median']:10.0f} ({row['solo']['min']:.0f} .. {row['solo']['max']:.0f})   batch / solo = {row['speedup']:.2f}   "
              f"terminal launches {row['terminal_launches']}", file=sys.stderr, flush=True)
        batch.close()
        for d in solos + batch.members:
            d.close()
    result = dict(tool="terminal_batch_bench", lattice=args.lattice, device=torch.cuda.get_device_name(0), locate=locate, rows=rows)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
