"""Throughput of a batch of small problems against the same problems solved one after another.

    python tools/batch_bench.py [--sizes 1,2,4,8,16,32,64] [--iters 200] [--reps 5] [--out profiles/batch/result.json]

B copies of benchmark4, each with its own rho in [0.5, 2] so that the copies do not run in lock-step, and with the stop test
switched off (eps_abs = eps_rel = 0) so that every run is exactly ``--iters`` iterations of every problem.  Three ways to do that
work, alternated inside every repetition (other work shares the host; profiles/batch/README.md has the table):
  batch   one BatchSolver: per iteration one vertex launch and one edge + control launch for all B problems
  (a)     the same B problems one after another, each on its own solo handle of the same program (workgroup256)
  (b)     one solo handle as gcsadmm_create plans it on its own (512 threads per workgroup), the B problems one after another
The rate is aggregate problem-iterations per second of wall time around work that ends in a device synchronise; medians of the
repetitions after one warm-up, with the spread (min .. max).  At B = 1 the device time per iteration (HIP events around the loop) of the
batch and of the solo handle is reported too: the cost of reading the arguments from a table instead of the kernarg segment
(per kernel: run this tool with ``--sizes 1`` under ``rocprofv3 --kernel-trace --stats``).  Needs the GPU; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,2,4,8,16,32,64")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", default="benchmark4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gcs_admm_amd import BatchSolver, load_fixture
    from gcs_admm_amd.solver import DeviceSolver
    assert torch.cuda.is_available(), "batch_bench needs a GPU"
    g = load_fixture(args.case)[1]
    K = args.iters
    fixed = dict(eps_abs=0.0, eps_rel=0.0, max_it=K + 1)
    sync = lambda: torch.cuda.synchronize(0)
    auto = DeviceSolver(g, "f64", device=0)
    rows = []
    for B in [int(s) for s in args.sizes.split(",")]:
        rhos = [1.0] if B == 1 else [float(r) for r in np.linspace(0.5, 2.0, B)]
        params = [dict(rho=r) for r in rhos]
        batch = BatchSolver([g] * B, "f64", device=0)
        solos = [DeviceSolver(g, "f64", device=0, program="workgroup256") for _ in range(B)]

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

        def run_auto():
            dt = 0.0
            for p in params:
                auto.reset(**p, **fixed)
                sync(); t0 = time.perf_counter()
                auto.enqueue(K)
                assert auto.read_control().it == K + 1
                dt += time.perf_counter() - t0
            return dt

        def device_ms(reset, enqueue):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync(); e0.record(); enqueue(K); e1.record(); sync()
            return e0.elapsed_time(e1) / K

        ways = dict(batch=run_batch, solo_wg256=run_solos, solo_auto=run_auto)
        times = {k: [] for k in ways}
        for rep in range(args.reps + 1):
            for k, f in ways.items():
                dt = f()
                if rep > 0:       # the first round warms up every shape
                    times[k].append(dt)
        rate = lambda dts: [B * K / dt for dt in dts]
        row = dict(B=B, iters=K, reps=args.reps, workgroups=B * batch.members[0].query()["num_workgroup_vertices"] + B,
                   lds_bytes=batch.members[0].query()["workgroup_lds_bytes"])
        for k, dts in times.items():
            r = rate(dts)
            row[k] = dict(median=statistics.median(r), min=min(r), max=max(r))
        row["speedup_vs_solo_wg256"] = row["batch"]["median"] / row["solo_wg256"]["median"]
        row["speedup_vs_solo_auto"] = row["batch"]["median"] / row["solo_auto"]["median"]
        if B == 1:
            ms_b = [device_ms(lambda: batch.reset(params, **fixed), batch.enqueue) for _ in range(args.reps)]
            ms_s = [device_ms(lambda: solos[0].reset(**params[0], **fixed), solos[0].enqueue) for _ in range(args.reps)]
            row["device_us_per_iteration"] = dict(batch=1e3 * statistics.median(ms_b), solo_wg256=1e3 * statistics.median(ms_s))
        rows.append(row)
        print(f"B={B:3d}  batch {row['batch']['median']:10.0f} it/s ({row['batch']['min']:.0f} .. {row['batch']['max']:.0f})   "
              f"(a) solo wg256 {row['solo_wg256']['median']:10.0f} ({row['solo_wg256']['min']:.0f} .. {row['solo_wg256']['max']:.0f})   "
              f"(b) solo auto {row['solo_auto']['median']:10.0f} ({row['solo_auto']['min']:.0f} .. {row['solo_auto']['max']:.0f})   "
              f"batch / (a) = {row['speedup_vs_solo_wg256']:.2f}", file=sys.stderr, flush=True)
        batch.close()
        for d in solos:
            d.close()
    result = dict(tool="batch_bench", case=args.case, device=torch.cuda.get_device_name(0), rows=rows)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
