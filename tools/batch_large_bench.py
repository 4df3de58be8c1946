"""Throughput of a batch of LARGE problems (``BatchSolver(..., large=True)``, GCSADMM_BATCH_LARGE) against the same problems solved one
after another, and against the same batch forced onto the workgroup program.

    python tools/batch_large_bench.py [--lattices 25x40,60x60] [--sizes 1,2,4,8,16] [--iters 400] [--reps 5] [--scene 4,16]
                                      [--out profiles/batch_large/result.json]

B copies of a brick lattice of ``graph.lattice_boxes``, each with its own rho in [0.5, 2] so that the copies do not run in lock-step,
and with the stop test switched off (eps_abs = eps_rel = 0) so that every run is exactly ``--iters`` iterations of every problem.  Three
ways to do that work, alternated inside every repetition (other work shares the host; profiles/batch_large/README.md has the table):
  (a)     one large batch, every member on the program ``batch.member_programs`` chooses (above 1 024 generic vertices in the whole
          batch: the wavefront program, packed by the batch's total)
  (b)     the same B problems one after another on a solo handle as gcsadmm_create plans it on its own: the only way without the flag
  (c)     one large batch with every member forced to ``program="workgroup256"``
The rate is aggregate problem-iterations per second of wall time around work that ends in a device synchronise; medians of the
repetitions after one warm-up, with the spread (min .. max).  Before anything is timed every member of (a) is compared bit for bit with a
solo handle of the same knobs after ``--iters`` iterations (state and trace); a difference ends the run.  ``--scene``: wall time of
``SceneQueries.solve(large=True)`` on the 25 x 40 scene with that many unpruned local queries.  Needs the GPU; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STATE = ("copy", "mu", "zedge", "xv", "zv", "yv")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", default="25x40,60x60")
    ap.add_argument("--sizes", default="1,2,4,8,16")
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scene", default="4,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gcs_admm_amd import BatchSolver
    from gcs_admm_amd.batch import member_programs
    from gcs_admm_amd.graph import lattice_boxes
    from gcs_admm_amd.solver import DeviceSolver
    assert torch.cuda.is_available(), "batch_large_bench needs a GPU"
    K = args.iters
    fixed = dict(eps_abs=0.0, eps_rel=0.0, max_it=K + 1)
    sync = lambda: torch.cuda.synchronize(0)
    rows = []
    for lattice in [s for s in args.lattices.split(",") if s]:
        nx, ny = (int(v) for v in lattice.split("x"))
        g = lattice_boxes(nx, ny)
        auto = DeviceSolver(g, "f64", device=0)
        for B in [int(s) for s in args.sizes.split(",")]:
            rhos = [1.0] if B == 1 else [float(r) for r in np.linspace(0.5, 2.0, B)]
            params = [dict(rho=r) for r in rhos]
            knobs = member_programs([g] * B, large=True)
            batch = BatchSolver([g] * B, "f64", device=0, large=True)
            forced = BatchSolver.of([DeviceSolver(g, "f64", device=0, program="workgroup256") for _ in range(B)], large=True)

            # (a) equals its solos, bit for bit: checked once, outside the timing
            batch.reset(params, **fixed)
            batch.enqueue(K)
            sync()
            for i in range(B):
                d = DeviceSolver(g, "f64", device=0, **knobs[i])
                d.reset(**params[i], **fixed)
                d.enqueue(K)
                sync()
                for f in STATE + ("trace",):
                    if getattr(d, f).cpu().numpy().tobytes() != getattr(batch.members[i], f).cpu().numpy().tobytes():
                        raise SystemExit(f"{lattice} B={B} member {i}: `{f}` of the batch differs from the solo handle's")
                d.close()

            def run(b):
                b.reset(params, **fixed)
                sync(); t0 = time.perf_counter()
                b.enqueue(K)
                status, it = b.poll()
                dt = time.perf_counter() - t0
                assert all(i == K + 1 for i in it), it
                return dt

            def run_auto():
                dt = 0.0
                for p in params:
                    auto.reset(**p, **fixed)
                    sync(); t0 = time.perf_counter()
                    auto.enqueue(K)
                    assert auto.read_control().it == K + 1
                    dt += time.perf_counter() - t0
                return dt

            ways = dict(large=lambda: run(batch), solo_auto=run_auto, large_wg256=lambda: run(forced))
            times = {k: [] for k in ways}
            for rep in range(args.reps + 1):
                for k, f in ways.items():
                    dt = f()
                    if rep > 0:       # the first round warms up every shape
                        times[k].append(dt)
            row = dict(lattice=lattice, B=B, iters=K, reps=args.reps, member_knobs=knobs[0], launches=batch.launches(),
                       launches_wg256=forced.launches(), solo_auto_plan=auto.query())
            for k, dts in times.items():
                r = [B * K / dt for dt in dts]
                row[k] = dict(median=statistics.median(r), min=min(r), max=max(r))
            row["large_over_solo_auto"] = row["large"]["median"] / row["solo_auto"]["median"]
            row["large_over_large_wg256"] = row["large"]["median"] / row["large_wg256"]["median"]
            rows.append(row)
            show = lambda k: f"{row[k]['median']:9.0f} ({row[k]['min']:.0f} .. {row[k]['max']:.0f})"
            print(f"{lattice} B={B:3d} {knobs[0]}  (a) large {show('large')}   (b) solo auto {show('solo_auto')}   (c) large wg256 {show('large_wg256')}   "
                  f"(a)/(b) = {row['large_over_solo_auto']:.2f}  (a)/(c) = {row['large_over_large_wg256']:.2f}", file=sys.stderr, flush=True)
            for b in (batch, forced):
                b.close()
                for m in b.members:
                    m.close()
        auto.close()
    scene = []
    counts = [int(s) for s in args.scene.split(",") if s]
    if counts:
        from gcs_admm_amd.queries import SceneQueries
        nx, ny = 25, 40
        g = lattice_boxes(nx, ny)
        cells = range(2, g.num_vertices)
        As = {("cell", v - 2): g.poly_A[g.poly_ptr[v]:g.poly_ptr[v + 1]] for v in cells}
        bs = {("cell", v - 2): g.poly_b[g.poly_ptr[v]:g.poly_ptr[v + 1]] for v in cells}
        rng = np.random.default_rng(nx * ny)
        with SceneQueries(As, bs, 2) as sq:
            for Q in counts:
                i, j = rng.integers(0, nx - 2, Q), rng.integers(0, ny - 3, Q)
                S, G = sq.centers[j * nx + i], sq.centers[(j + 3) * nx + i + 2]
                ts = []
                for rep in range(args.reps + 1):
                    sync(); t0 = time.perf_counter()
                    rec = sq.solve(S, G, large=True)
                    if rep > 0:
                        ts.append(time.perf_counter() - t0)
                line = dict(queries=Q, regions=nx * ny, solve_s=statistics.median(ts), solve_s_spread=[min(ts), max(ts)],
                            iterations=[int(r["iterations"]) for r in rec], status=[r["status"] for r in rec],
                            rounded_cost=[float(r["rounded_cost"]) for r in rec])
                scene.append(line)
                print(f"SceneQueries.solve(large=True), {Q} unpruned queries on {nx}x{ny}: {line['solve_s']:.3f} s "
                      f"({min(ts):.3f} .. {max(ts):.3f}), iterations {line['iterations']}", file=sys.stderr, flush=True)
    result = dict(tool="batch_large_bench", device=torch.cuda.get_device_name(0), rows=rows, scene=scene)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
