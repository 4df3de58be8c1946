"""The rounding step of a batch of queries with the walks on the host and on the device.

    python tools/rounding_bench.py [--sizes 1,8,64] [--case benchmark4] [--reps 5] [--out profiles/walks/rounding_bench.jsonl]

B copies of the query of one committed benchmark (its own terminals on its own regions; every copy rounds with its own seed), solved
ONCE by ``SceneQueries.graphs`` + ``BatchSolver.solve``; the members stay open, and the rounding of all B of them is timed both ways
on the same activations:
  host     ``rounding_problem`` per member (the activations to the host, one dict entry per edge) + ``rounding_many``
  device   ``rounding_members``: one ``DeviceWalks.sample`` for all members, no per-edge Python object
Both end in the same batched path restrictions on the device (one scene over the concatenated regions, one call per round); the candidate
paths differ, since the two walks follow different rules.  Wall time around work that ends synchronised; the two sides alternate inside
every repetition, median of ``--reps`` after one warm-up, with the spread.  ``before_restriction`` is the part of a run spent before its
first restriction call: for the host side the copies, the dicts, the scene upload and the first round of walks; for the device side
the walk upload and launch, the scene upload and the candidate bookkeeping.  No kernel time is taken here (run under ``rocprofv3
--kernel-trace --stats`` for that).  Needs the GPU; prints one JSON line per B."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--case", default="benchmark4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gcs_admm_amd import BatchSolver, SceneQueries, rounding
    from gcs_admm_amd.cases import fixture_sets
    from gcs_admm_amd.graph import sets_of_graph
    assert torch.cuda.is_available(), "rounding_bench needs a GPU"
    As_all, bs_all, n, _, _ = fixture_sets(args.case)
    point = lambda k: (np.asarray(bs_all[k])[:n] - np.asarray(bs_all[k])[n:]) / 2        # a terminal is the box around its point
    As = {k: A for k, A in As_all.items() if k not in ('s', 't')}
    bs = {k: bs_all[k] for k in As}
    first_call = []
    device_solver = rounding.solve_path_restrictions_device

    def stamped(*a, **kw):
        if not first_call:
            first_call.append(time.perf_counter())
        return device_solver(*a, **kw)
    rounding.solve_path_restrictions_device = stamped
    lines = []
    with SceneQueries(As, bs, n) as sq:
        for B in [int(s) for s in args.sizes.split(",")]:
            graphs = sq.graphs(np.array([point('s')] * B), np.array([point('t')] * B))
            seeds = list(range(B))
            batch = BatchSolver(graphs, "f64", device=0)
            records = batch.solve()

            def host():
                problems = [rounding.rounding_problem(m, *sets_of_graph(g), seed=s) for m, g, s in zip(batch.members, graphs, seeds)]
                return rounding.rounding_many(problems, device=0)

            def device():
                return rounding.rounding_members(batch.members, graphs, seeds=seeds, device=0)
            ways = dict(host=host, device=device)
            total = {k: [] for k in ways}
            before = {k: [] for k in ways}
            costs = {}
            for rep in range(args.reps + 1):
                for k, f in ways.items():
                    del first_call[:]
                    torch.cuda.synchronize(0); t0 = time.perf_counter()
                    out = f()
                    torch.cuda.synchronize(0); t1 = time.perf_counter()
                    costs[k] = [c for c, _, _ in out]
                    if rep > 0:      # the first round warms up both sides
                        total[k].append(t1 - t0); before[k].append((first_call[0] if first_call else t1) - t0)
            batch.close()
            for m in batch.members:
                m.close()
            ms = lambda xs: dict(median=1e3 * statistics.median(xs), min=1e3 * min(xs), max=1e3 * max(xs))
            row = dict(tool="rounding_bench", case=args.case, device=torch.cuda.get_device_name(0), B=B, reps=args.reps,
                       vertices=graphs[0].num_vertices, edges=[g.num_edges for g in graphs][:4], converged=sum(r["status"] == "converged" for r in records),
                       host_ms=ms(total["host"]), device_ms=ms(total["device"]),
                       host_before_restriction_ms=ms(before["host"]), device_before_restriction_ms=ms(before["device"]),
                       finite_costs=dict(host=int(np.isfinite(costs["host"]).sum()), device=int(np.isfinite(costs["device"]).sum())),
                       worst_relative_cost_difference=float(max((abs(a - b) / a for a, b in zip(costs["host"], costs["device"]) if np.isfinite(a) and np.isfinite(b)),
                                                                 default=0.0)))
            row["host_over_device"] = row["host_ms"]["median"] / row["device_ms"]["median"]
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
