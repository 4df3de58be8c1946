#!/usr/bin/env python3
"""bench.py -- ADMM iterations/sec of the MI355X loop, one JSON line on stdout.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload benchmark4|s10k|s100k|s6d] [--dump-outputs DIR] [--full]

A "step" is one full ADMM iteration (vertex step, edge step, control: admm_solver_v3.py:655-733) on the resident state; K steps are
enqueued back to back (no host round trip) between two synchronisation points.  The state is already in HBM when the timed region
starts: the loop is first advanced, untimed, to `config.window.first_iteration` (the vertex solves restart from the previous
iteration's records -- csrc/warm_start.h -- so the cost of an iteration depends on where in the run it lies).

A plain run does only what the headline needs: it sets up, advances the loop to the window, runs the W warm-up and the K timed steps,
writes --dump-outputs and prints the line (`value`, `ms_per_step`, `config`).  Everything else described below -- the whole run to the
stop, the CPU oracle, the rooflines, the other configs, the sharded leg on one rank; at N > 1 the per-stage shares, the one-GPU
comparison, the strip model and the benchmark4 replicas -- is measured only with --full (--no-cpu, --no-configs and --loop-only trim
a --full run).

N = 1 (default): the configuration BASELINE.json quotes its metric on, benchmark4 in f64.  The window is CENTRED on the run to the
reference's own stop (465 iterations: no tuned parameter); `value_to_stop` is the rate over the WHOLE run from the zero state to the
reference's stop rule (median of three runs).  `cpu_baseline` times the CPU oracle (oracle/gcs_oracle.c, "port", same warm start of
the vertex solves) on the host cores over THE SAME iteration window -- advanced untimed to the same first iteration, the same K
iterations timed, every part of the iteration on both sides -- and over the same whole run (`to_stop`).  `roofline` prices the
dominant kernel (vertex step) with the algorithmic bytes of SURVEY.md section 8(d); its launch time is the timed window's time per
step times the kernel's share of the device time (HIP events on the launch stream in a replay of the same window).  The line also
carries compact blocks for BASELINE configs 3 and 5 (`configs.s10k`, `configs.s6d`) and the sharded loop of config 4 on one rank.

N > 1: `python bench.py --gpus N` starts N fresh rank processes itself (torch.distributed.run as a child, before this process has
touched a GPU) unless it already runs under a launcher (WORLD_SIZE set), and relays rank 0's line.  The headline is then the SHARDED
path, the fan-out that replaces SolveInParallel at admm_solver_v3.py:490: BASELINE config 4's 316 x 317 lattice (100k vertices) in N
row strips, the loop entirely behind the C ABI (gcsadmm_run_partitioned: RCCL halo exchange + 6-double all-reduce on one stream),
`scaling: "strong"`, with the same lattice on one GPU measured beside it.  benchmark4 (42 vertices) does not shard; N independent
replicas of it are a side field (`replicas_benchmark4`).

--dump-outputs DIR: after the timed steps, what the timed loop computed in its last step (the state a caller of the loop receives,
the control scalars and the K timed trace rows) as DIR/<name>.npy, at most 64 MB in all; the inputs are fixed (fixture, seeded
lattices), so two builds run with the same arguments can be compared array for array.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from gcs_admm_amd import IPM_TOL  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
F64_VECTOR_PEAK_TF = 78.6      # MI355X f64 vector peak (spec)
REF_PUBLISHED_ITS = 465 / 37.87852382659912   # v3 / benchmark4, solver-time-only, hardware unknown
PROFILE_DIR = os.path.join(ROOT, "profiles", "r04")
REFERENCE_STOP_B4 = 465        # iterations of the reference's own run of benchmark4 (benchmark_data/admm_solver_v3_benchmark4.pkl)
# iterations run untimed before the warm-up.  benchmark4: the window of W + K iterations is centred on the run to the reference's stop
# (window_start); the synthetic configs have no reference run: a fixed start in the body of the run (past the rho adaptation's first moves)
WINDOW_START = {"s10k": 150, "s100k": 60, "s6d": 60}


def window_start(workload, warmup, steps):
    if workload == "benchmark4":
        return max((REFERENCE_STOP_B4 - (warmup + steps)) // 2, 0)
    return WINDOW_START[workload]


def make_workload(name):
    from gcs_admm_amd.cases import load_fixture
    from gcs_admm_amd.graph import lattice_boxes
    if name == "benchmark4":
        case, g = load_fixture("benchmark4")
        return g, "f64", dict(case=case)
    if name == "s10k":       # BASELINE config 3
        return lattice_boxes(100, 100, seed=0), "f32", {}
    if name == "s100k":      # BASELINE config 4's graph on one GPU
        return lattice_boxes(316, 317, seed=0), "f32", {}
    if name == "s6d":        # BASELINE config 5
        return lattice_boxes(223, 224, n=6, seed=0), "f32", {}
    raise SystemExit(f"unknown workload {name}")


class stdout_to_stderr:
    """RCCL prints a version banner on stdout when a communicator is created; stdout carries the one JSON line only"""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)


def time_window(dev, first, warmup, steps, enqueue=None, barrier=None):
    """advance the loop untimed to iteration `first`, W warm-up steps, then K timed steps between two synchronisations"""
    import torch
    enqueue = enqueue or dev.enqueue
    dev.reset(max_it=first + warmup + steps + 1, eps_abs=0.0, eps_rel=0.0)      # stop test off: exactly K iterations run
    if first + warmup > 0:
        enqueue(first + warmup)
    torch.cuda.synchronize()
    if barrier:
        barrier()
    t0 = time.perf_counter()
    enqueue(steps)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


DUMP_CAP_BYTES = 64 << 20      # --dump-outputs: at most 64 MB in all


def loop_outputs(dev, first, warmup, steps):
    """What the timed loop hands its caller after its last step, as host arrays: the vertex solution (x_v, z_v, y_v), the edge
    variables, the copies and the duals (pending mu scale applied) in incidence order -- the numbering that does not depend on the
    state layout --, the control scalars after the last step and the trace rows of the K timed iterations (row it - 1 = iteration it)."""
    import numpy as np
    cb = dev.read_control()
    host = lambda t: t.cpu().numpy()
    E, col = dev.g.num_edges, dev.col_of
    rows = slice(first + warmup, first + warmup + steps)
    mu = host(dev.mu)[:, col]
    return {"x_v": host(dev.xv), "z_v": host(dev.zv), "y_v": host(dev.yv), "z_edge": host(dev.zedge)[:, :E],
            "copy": host(dev.copy)[:, col], "mu": mu * mu.dtype.type(cb.mu_scale),
            "control": np.array([cb.it, cb.status, cb.rho, cb.mu_scale, cb.pri, cb.dual, cb.eps_pri, cb.eps_dual, cb.inner_failures],
                                dtype=np.float64),
            "trace": host(dev.trace[rows])}


def dump_outputs(arrays, dirname, cap=DUMP_CAP_BYTES):
    """DIR/<name>.npy for every array (float32 / float64 as computed).  Over `cap` bytes in all, every array of more than 1 MB keeps
    the same share of its longest axis: a sorted sample drawn with a seed fixed by that axis' length, so that arrays sharing an axis
    (copy and mu) keep the same columns and the same arguments give the same sample on every run."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    big = lambda a: a.nbytes > (1 << 20)
    small = sum(a.nbytes for a in arrays.values() if not big(a)) + 4096 * len(arrays)      # (room for the .npy headers)
    large = sum(a.nbytes for a in arrays.values() if big(a))
    share = min(1.0, (cap - small) / large) if large else 1.0
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        if share < 1.0 and big(a):
            ax = int(np.argmax(a.shape))
            idx = np.sort(np.random.default_rng(a.shape[ax]).choice(a.shape[ax], max(int(a.shape[ax] * share), 1), replace=False))
            a = np.take(a, idx, axis=ax)
        np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(a))


def kernel_shares(dev, first, warmup, steps):
    """device time of the two kernels over a replay of the same window (HIP events around every launch, on the launch stream).
    The events serialise the launches, so only the RATIO of the two is used."""
    dev.reset(max_it=first + warmup + steps + 1, eps_abs=0.0, eps_rel=0.0)
    if first + warmup > 0:
        dev.enqueue(first + warmup)
    tm = dev.enqueue_timed(steps)
    tot = tm["vertex_ms"] + tm["edge_ms"]
    cb = dev.read_control()
    return tm["vertex_ms"] / tot, tm["edge_ms"] / tot, cb, tm


def cpu_baseline(g, workload, first, warmup, steps, seconds=20.0, dev=None, to_stop=False):
    """The oracle on the host cores over THE SAME iteration window as the GPU (same iteration window, same run, all of
    admm_solver_v3.py:655-733 on both sides): the loop is advanced untimed through iterations 1 .. first + W (oracle_admm_run_from
    keeps the reference's iteration numbering, so the rho adaptation sees the same counter), the state and the warm-start records
    are snapshotted, and iterations first + W + 1 .. first + W + K are timed; the window is repeated from the snapshot for about
    `seconds` of CPU work at the best thread count of a short sweep on that same window; `value` is the median repetition.
    Where advancing from the zero state would not fit a bounded sample (S6D: about 1 it/s on 64 cores) the state at iteration
    `first` is transplanted from the GPU run (`dev`) instead and the W warm-up iterations (at least 3) rebuild the oracle's
    warm-start records before the timed K -- `state_preparation` says which.  to_stop: also time the whole run from the zero state
    to the reference's stop rule (median of three)."""
    import numpy as np
    from oracle.oracle import Oracle
    ncpu = os.cpu_count() or 1
    o = Oracle(g, ipm_tol=IPM_TOL)
    transplant = dev is not None
    rho = 1.0
    if transplant:      # GPU state after `first` iterations -> oracle layout (incidence-major f64, pending mu rescale applied)
        dev.reset(max_it=first + warmup + steps + 1, eps_abs=0.0, eps_rel=0.0)
        if first > 0:
            dev.enqueue(first)
        cb = dev.read_control()
        col = dev.col_of
        o.copy[...] = dev.copy.double().cpu().numpy()[:, col]
        o.mu[...] = cb.mu_scale * dev.mu.double().cpu().numpy()[:, col]
        o.zedge[...] = dev.zedge.double().cpu().numpy()
        rho = float(cb.rho)
        warmup_cpu = max(warmup, 3)
        prep = (f"state of the GPU run after {first} iterations transplanted into the oracle; {warmup_cpu} untimed warm-up iterations "
                "rebuild its warm-start records (advancing the oracle from the zero state would take minutes at this size)")
    else:
        warmup_cpu = warmup
        prep = f"oracle advanced untimed from the zero state through iterations 1..{first + warmup}"
    th0 = min(ncpu, 32)
    w_first = first + warmup + 1                       # first timed iteration (the GPU's numbering)
    a0 = first + warmup - warmup_cpu + 1               # (transplant: the warm-up runs as iterations a0 .. first + W)
    if (first + warmup if not transplant else warmup_cpu) > 0:
        _, _, rho, _ = o.run_from(1 if not transplant else a0, first + warmup, rho=rho, eps_abs=0.0, eps_rel=0.0, nthreads=th0)
    snap = o.snapshot()

    def window(th):
        o.restore(snap)
        t0 = time.perf_counter()
        it, _, _, _ = o.run_from(w_first, first + warmup + steps, rho=rho, eps_abs=0.0, eps_rel=0.0, nthreads=th)
        dt = time.perf_counter() - t0
        assert it == first + warmup + steps + 1, it
        return steps / dt
    # thread count: best of a short sweep on the window itself
    t_budget = time.perf_counter()
    rates = {}
    # (the plausible counts first: the sweep stops when its share of the budget is spent; one thread only where it costs little)
    order = [th for th in (32, 64, 16, 128, 8, ncpu, 1) if th <= ncpu]
    for th in dict.fromkeys(order):
        if th == 1 and g.num_vertices > 1000 and ncpu > 1:
            continue
        rates[th] = window(th)
        if g.num_vertices < 1000 and rates[th] > 0.3 * max(rates.values()):      # (small graphs: noisy, best of three -- unless the count is hopeless)
            rates[th] = max(rates[th], window(th), window(th))
        if time.perf_counter() - t_budget > 0.6 * seconds and len(rates) >= 2:
            break
    cores = max(rates, key=rates.get)
    reps = [rates[cores]]
    while time.perf_counter() - t_budget < seconds and len(reps) < 400:
        reps.append(window(cores))
    out = {"value": float(np.median(reps)), "unit": "iterations/s", "cores": cores, "kind": "port", "host_cpus": ncpu,
           "window": {"first_iteration": w_first, "last_iteration": first + warmup + steps},
           "state_preparation": prep, "repetitions": len(reps), "selection": "median of the repetitions", "best_repetition": float(max(reps)),
           "thread_sweep": {str(k): v for k, v in rates.items()},
           "single_thread_value": rates.get(1),
           "sample": f"iterations {w_first}..{first + warmup + steps} of the same run (oracle/gcs_oracle.c: vertex solves with the same warm start as the "
                     f"HIP path, OpenMP over vertices; edge step, dual update, norms and loop control serial, as in the reference), the window repeated "
                     f"{len(reps)} x from a snapshot, {cores} threads (best of a sweep up to {ncpu})"}
    if to_stop:      # the whole run from the zero state to the reference's stop rule: its own thread sweep (the best count for a 20-iteration
        # window of cheap solves is not the best for a run that starts with cold ones), median of three runs at each count
        best = None
        for th in sorted(rates):
            if rates[th] < 0.3 * max(rates.values()) and th != 1:      # (an oversubscribed count -- 256 threads: 8 it/s on the window -- would take minutes here)
                continue
            runs = []
            for _ in range(3):
                oo = Oracle(g, ipm_tol=IPM_TOL)
                t0 = time.perf_counter()
                r = oo.run(nthreads=th)
                runs.append((time.perf_counter() - t0, r["iterations"]))
                if runs[-1][0] > 2.0:      # bounded sample: a count this slow cannot be the best
                    break
            runs.sort()
            if len(runs) < 3:
                continue
            if best is None or runs[1][0] < best[1][1][0]:
                best = (th, runs)
        th, runs = best
        out["to_stop"] = {"iterations": runs[1][1], "wall_time_s": runs[1][0], "iterations_per_sec": runs[1][1] / runs[1][0], "cores": th,
                          "runs": 3, "selection": "median wall time at the best thread count of the sweep", "all_wall_times_s": [r[0] for r in runs]}
    return out


def measured_traffic(workload, family):
    """HBM bytes per launch of a kernel family ("vertex" / "edge") of this workload.  PMC counters cannot be read from inside this
    process: the figure is the one rocprofv3 collected for this same command line (separate --pmc passes, tools/profile_round.sh ->
    profiles/r04), FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950, KB -> bytes.  (None, None) when no profile of
    the workload is committed."""
    prof = os.path.join(PROFILE_DIR, f"{workload}_hbm_counters.json")
    if not os.path.exists(prof):      # no profile of this round yet: the last committed one of an earlier round
        older = sorted(p_ for p_ in (os.path.join(ROOT, "profiles", d, f"{workload}_hbm_counters.json") for d in os.listdir(os.path.join(ROOT, "profiles")))
                       if os.path.exists(p_))
        if not older:
            return None, None
        prof = older[-1]
    pc = json.load(open(prof))
    kk = next((k for k in pc.get("FETCH_SIZE", {}) if k == family or (family == "edge" and k.startswith("edge"))), None)
    if not kk or kk not in pc.get("WRITE_SIZE", {}):
        return None, None
    return 1024.0 * (2.0 * pc["FETCH_SIZE"][kk]["mean_KB_per_launch"] + pc["WRITE_SIZE"][kk]["mean_KB_per_launch"]), os.path.relpath(prof, ROOT)


def counted_flops(g):
    """f64 operations of ONE cold vertex step from the zero state, counted (not modelled): the workgroup program's source
    compiled for the host with a counting scalar type (tools/flopcount), add / mul = 1, fma = 2, division and square root
    listed apart.  None when the counter is not built."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools", "flopcount"))
        import wg_flops
        return wg_flops.count_vertex_step(g)
    except Exception:      # tooling, never the product: its absence only drops the field
        return None


def rooflines(g, dtype, q, program, workload, ms_per_step, share_v, share_e, cb, columns, with_flops):
    """the three roofline objects of one workload from its window time per step and the kernels' shares of it"""
    wb = 8 if dtype == "f64" else 4
    v_ms, e_ms = ms_per_step * share_v, ms_per_step * share_e
    alg_bytes = g.algorithmic_bytes_per_iteration(wb)
    ach = alg_bytes / (v_ms * 1e-3) / 1e9
    kernel = {"workgroup": f"vertex_wg_kernel<{g.n}>", "wavefront": "vertex_kernel<2>", "mixed": "vertex_kernel<2> + vertex_wg_kernel<2>"}[program]
    traffic, traffic_src = measured_traffic(workload, {"workgroup": "vertex_wg_kernel", "wavefront": "vertex_kernel"}.get(program, "-"))
    n_generic = g.num_vertices - q["num_special"]
    it_per_vertex = cb.inner_iters / max(n_generic, 1)
    out = {"roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                        "traffic": traffic, "traffic_source": traffic_src, "kernel": kernel, "avg_launch_ms": v_ms,
                        "avg_launch_ms_source": "ms_per_step x the kernel's share of the device time (HIP events on the launch stream, replay of the window)",
                        "algorithmic_bytes_per_launch": alg_bytes, "edge_step_avg_ms": e_ms,
                        "waves": q["num_waves"], "lds_bytes_per_wave": q["lds_bytes"],
                        "workgroup_vertices": q["num_workgroup_vertices"], "lds_bytes_per_workgroup": q["workgroup_lds_bytes"],
                        "newton_iterations_per_vertex": it_per_vertex, "special_vertices": q["num_special"],
                        "note": "the vertex step is bound by dependent f64 issue / LDS latency, not by HBM (DESIGN.md section 4): "
                                "the HBM fraction on algorithmic bytes is reported as SURVEY 8(d) asks; see roofline_fp"}}
    fl = counted_flops(g) if with_flops else None
    if fl is not None:
        # counted on a cold step from the zero state, scaled to this window's Newton iterations per vertex
        scale = it_per_vertex / max(fl["newton_iterations_per_vertex"], 1e-9)
        flops = fl["flops"] * scale
        out["roofline_fp"] = {"bound": "f64 vector", "achieved": flops / (v_ms * 1e-3) / 1e12, "peak": F64_VECTOR_PEAK_TF, "unit": "TFLOP/s",
                              "frac": flops / (v_ms * 1e-3) / 1e12 / F64_VECTOR_PEAK_TF, "flops_per_launch": flops,
                              "divisions_per_launch": fl["div"] * scale, "sqrt_per_launch": fl["sqrt"] * scale,
                              "counted_on": "workgroup program" + ("" if program == "workgroup" else
                                                                   " (WORKGROUP-PROGRAM-EQUIVALENT: this workload runs the wavefront program, whose own operation count is not instrumented)"),
                              "note": "COUNTED f64 operations of the vertex step (tools/flopcount: the workgroup program's source "
                                      "compiled for the host with a counting scalar; add/mul = 1, fma = 2), scaled to this "
                                      "window's Newton iterations per vertex"}
    # the streaming half of the iteration on its own (edge average + dual + residual sums + control).  Bytes of THIS layout:
    # read 2 copies + 2 mu + zedge (5c), write zedge + 2 mu (3c) -- targets are never stored, so this is
    # below the 10c words SURVEY 8(d) budgets for an edge kernel that writes them.  HBM-bound once the state outgrows the caches.
    edge_bytes = 8.0 * g.c * g.num_edges * wb
    out["roofline_edge"] = {"bound": "hbm", "achieved": edge_bytes / (e_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": edge_bytes / (e_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "kernel": "edge_kernel (one launch: averages, duals, norms, control)",
                            "avg_step_ms": e_ms, "algorithmic_bytes_per_step": edge_bytes,
                            "traffic": measured_traffic(workload, "edge")[0], "state_columns": columns}
    return out


def config_block(name, steps, warmup, local, cpu, cpu_seconds=8.0):
    """compact block of another BASELINE config for the default line: window rate, kernels, rooflines, stop, CPU oracle (same window)"""
    import torch
    from gcs_admm_amd.solver import DeviceSolver
    g, dtype, _ = make_workload(name)
    columns = "edge" if g.num_edges >= 20000 else "incidence"
    dev = DeviceSolver(g, dtype, device=local, columns=columns)
    q = dev.query()
    program = "workgroup" if q["num_workgroup_vertices"] and not q["num_waves"] else ("wavefront" if not q["num_workgroup_vertices"] else "mixed")
    first = window_start(name, warmup, steps)
    el = time_window(dev, first, warmup, steps)
    sv, se, cb, _ = kernel_shares(dev, first, warmup, steps)
    ms = 1e3 * el / steps
    blk = {"workload": name, "V": g.num_vertices, "E": g.num_edges, "n": g.n, "state_dtype": dtype, "state_columns": columns,
           "vertex_program": program, "iterations_per_sec": steps / el, "ms_per_step": ms, "steps": steps, "warmup": warmup,
           "window": {"first_iteration": first + warmup + 1, "last_iteration": first + warmup + steps}}
    blk.update(rooflines(g, dtype, q, program, name, ms, sv, se, cb, columns, with_flops=True))
    if name == "s10k":       # BASELINE config 3's second half: the reference's own stop rule (defaults) on the f32 state
        res = dev.solve(chunk=100)
        blk["convergence"] = {"iterations_to_stop": res["iterations"], "status": res["status"], "cost": res["cost"],
                              "loop_wall_time_s": res["wall_time_s"], "inner_failures": res["inner_failures"],
                              "iterations_per_sec_to_stop": res["iterations"] / max(res["wall_time_s"], 1e-12)}
    if cpu:
        blk["cpu_baseline"] = cpu_baseline(g, name, first, warmup, steps, seconds=cpu_seconds, dev=dev if g.num_vertices > 20000 else None)
        blk["gpu_over_cpu_same_window"] = blk["iterations_per_sec"] / blk["cpu_baseline"]["value"]
    dev.close()
    del dev
    torch.cuda.empty_cache()
    return blk


def strip_model(gl, local):
    """the static model the expected strong scaling of config 4 is argued from: wavefronts / workgroups
    of rank 0's strip at N = 1, 2, 4, 8 and the rounds of the chip's 1 024 one-wavefront-per-SIMD slots they need"""
    from gcs_admm_amd.partition import build_partition, strip_owner
    from gcs_admm_amd.solver import DeviceSolver
    rows = {}
    for n_ranks in (1, 2, 4, 8):
        part = build_partition(gl, strip_owner(gl, n_ranks), 0, n_ranks)
        d = DeviceSolver(part.graph, "f32", device=local, num_incidences=part.num_incidences, inc_counted=part.inc_counted,
                         edge_counted=part.edge_counted, nx_global=part.nx_global, nmu_global=part.nmu_global, columns="edge")
        q = d.query()
        rows[str(n_ranks)] = {"vertices": part.graph.num_vertices, "wavefronts": q["num_waves"], "rounds_of_1024_slots": -(-q["num_waves"] // 1024),
                              "cut_columns": int(sum(len(v) for v in part.send_idx.values()))}
        d.close()
    return rows


# ----------------------------------------------------------------------------------------------------------------------------------
# N ranks: started from here when no launcher did it (the driver's command form is `python bench.py --gpus N ...`)
# ----------------------------------------------------------------------------------------------------------------------------------
def launch_ranks(args, argv):
    """`--gpus N` with N > 1 and no WORLD_SIZE in the environment: start N fresh rank processes -- torch.distributed.run as a CHILD
    process, one rank per GPU, rendezvous on 127.0.0.1 -- before this process has initialised a GPU (it never does: no re-exec of a
    process that has touched the device), relay rank 0's JSON line and the children's exit code."""
    import socket
    import subprocess
    if not args.dry_launch:
        import torch      # (device_count() does not initialise the runtime)
        have = torch.cuda.device_count()
        if have < args.gpus:
            print(f"bench.py: --gpus {args.gpus} but {have} device(s) visible", file=sys.stderr)
            return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC (RCCL between processes)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)      # stderr passes through
    line = None
    for ln in proc.stdout.splitlines():
        ln = ln.strip()
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
    if line is not None:
        try:
            got = json.loads(line).get("n_gpus")
        except ValueError:
            got = None
        print(line, flush=True)
        if proc.returncode == 0 and got != args.gpus:
            print(f"bench.py: the ranks reported n_gpus = {got}, asked for {args.gpus}", file=sys.stderr)
            return 4
    elif proc.returncode == 0:
        print("bench.py: the ranks printed no result line", file=sys.stderr)
        return 5
    return proc.returncode


def dry_launch(args):
    """--dry-launch: what a rank sees after the launch, without touching a GPU (gloo): every rank reports its RANK / WORLD_SIZE /
    LOCAL_RANK, rank 0 prints them in one line shaped like the real one.  tests/test_bench_contract.py runs `--gpus 2 --dry-launch`."""
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1")); local = int(os.environ.get("LOCAL_RANK", "0"))
    seen = [[rank, world, local]]
    if world > 1:
        dist.init_process_group("gloo")
        t = torch.tensor([rank, world, local], dtype=torch.int64)
        got = [torch.zeros(3, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(got, t)
        seen = [[int(x) for x in g_] for g_ in got]
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "admm_iterations_per_sec", "dry_launch": True, "n_gpus": world, "gpus_argument": args.gpus,
                          "ranks": [{"rank": r, "world_size": w, "local_rank": l} for r, w, l in seen]}), flush=True)
    return 0


def sharded_leg(args, rank, world, local, steps, warmup, out, full, dump=None):
    """BASELINE config 4: ONE 316 x 317 lattice in `world` row strips, the loop behind the C ABI (gcsadmm_run_partitioned).  Collective:
    every rank calls it.  Returns (block, rank-0 extras) -- block is {} on ranks > 0.  `dump`: directory the timed loop's outputs
    of this rank's strip are written to (dump_outputs, names suffixed with the rank, an equal share of the cap per rank).  `full`:
    also the per-stage shares (a replay of the window), the strip model and, at N > 1, the same lattice on one GPU; without it the
    rank-0 extras `tm` and `pcb2` are None."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from gcs_admm_amd.solver import DeviceSolver
    block, ok = {}, 1.0
    watchdog = None
    if world > 1:
        # if a rank never reaches one of this leg's collectives the line is still printed (with the error named) instead of the job
        # hanging until the launcher's limit -- and the process fails
        import threading

        def leg_timed_out():
            if rank == 0:
                out["partitioned_s100k"] = {"error": f"timed out after {args.partition_timeout} s (a rank did not reach a collective of this leg)"}
                print(json.dumps(out), flush=True)
            os._exit(3)
        watchdog = threading.Timer(args.partition_timeout + (0 if rank == 0 else 20), leg_timed_out)
        watchdog.daemon = True
        watchdog.start()
    pfirst = WINDOW_START["s100k"]
    try:
        from gcs_admm_amd.graph import lattice_boxes
        from gcs_admm_amd.partition import device_partition
        gl = lattice_boxes(316, 317, seed=0)
        with stdout_to_stderr():
            part, pdev = device_partition(gl, rank, world, "f32", device=local, columns="edge")
    except Exception as exc:
        ok, block = 0.0, {"error": f"rank {rank}: {type(exc).__name__}: {exc}"}
    if world > 1:      # every rank learns whether ALL ranks are ready before the first collective of this leg
        flag = torch.tensor([ok], dtype=torch.float64, device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if ok and float(flag.item()) == 0.0:
            block = {"error": "another rank failed to set up its partition"}
        ok = float(flag.item())
    serial_rate = None
    if ok and world > 1:
        # the SERIAL schedule first (vertex step, exchange, edge step on one stream), and its rate into the line at once: should the
        # overlapped schedule -- two streams, never run with real neighbours before -- stall, the watchdog still prints a measured value
        pdev.set_overlap(2)
        sel_ = time_window(pdev, pfirst, warmup, steps, enqueue=pdev.enqueue_partitioned, barrier=dist.barrier)
        t = torch.tensor([sel_], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        serial_rate = steps / float(t.item())
        if rank == 0:
            out.update({"value": serial_rate, "ms_per_step": 1e3 * float(t.item()) / steps, "rccl_ranks": pdev.comm_count(),
                        "config": {"workload": "s100k", "window": {"first_iteration": pfirst + warmup + 1, "last_iteration": pfirst + warmup + steps},
                                   "parallelism": f"vertex partition: {world} row strips; SERIAL schedule (the overlapped one did not complete)"}})
        pdev.set_overlap(0)
    if ok:
        pel = time_window(pdev, pfirst, warmup, steps, enqueue=pdev.enqueue_partitioned, barrier=(dist.barrier if world > 1 else None))
        pcb = pdev.read_control()
        assert pcb.it == pfirst + warmup + steps + 1, (pcb.it, pcb.status)
        if dump:
            arrays = loop_outputs(pdev, pfirst, warmup, steps)
            dump_outputs({f"{k}_rank{rank}": v for k, v in arrays.items()}, dump, cap=DUMP_CAP_BYTES // world)
        halo = float(sum(len(v) for v in part.send_idx.values()))
        tm = pcb2 = None
        if full:      # per-stage device time of THIS rank over a replay of the window (events serialise nothing here: one stream)
            pdev.reset(max_it=pfirst + warmup + steps + 1, eps_abs=0.0, eps_rel=0.0)
            pdev.enqueue_partitioned(pfirst + warmup)
            tm = pdev.enqueue_partitioned_timed(min(steps, 100))
            pcb2 = pdev.read_control()
        ranks_rccl = pdev.comm_count()
        boundary_waves = pdev.set_overlap(0)      # (reads back the automatic choice: > 0 when this rank has neighbours and runs the wavefront program)
        if world > 1:
            t = torch.tensor([pel, halo], dtype=torch.float64, device="cuda")
            dist.all_reduce(t[:1], op=dist.ReduceOp.MAX); dist.all_reduce(t[1:], op=dist.ReduceOp.SUM)
            pel, halo = float(t[0].item()), float(t[1].item())
            cnt = torch.tensor([float(ranks_rccl)], dtype=torch.float64, device="cuda")
            dist.all_reduce(cnt, op=dist.ReduceOp.MIN)
            ranks_rccl = int(cnt.item())
        if rank == 0:
            q = pdev.query()
            block = {"workload": "s100k (316 x 317 box lattice, BASELINE config 4)", "V": gl.num_vertices, "E": gl.num_edges,
                     "partition": f"{world} row strip(s), one per GPU", "state_dtype": "f32", "scaling": "strong",
                     "iterations_per_sec": steps / pel, "ms_per_iteration": 1e3 * pel / steps, "iterations": int(pcb.it) - 1,
                     "steps": steps, "warmup": warmup,
                     "window": {"first_iteration": pfirst + warmup + 1, "last_iteration": pfirst + warmup + steps},
                     "halo_columns_per_iteration": int(halo), "halo_bytes_per_iteration": int(halo) * gl.c * 4,
                     "collectives_per_iteration": "1 grouped send/recv per neighbour + 1 all-reduce of 6 f64",
                     "rccl_ranks": ranks_rccl,
                     "communicator": (f"RCCL, {ranks_rccl} rank(s) by ncclCommCount: the all-reduce runs every iteration" if getattr(pdev, "has_comm", False)
                                      else "none (no all-reduce issued)"),
                     "path": "gcsadmm_run_partitioned (C ABI, RCCL on the caller's stream, no host synchronisation)",
                     "schedule": (f"overlapped: rank 0's {boundary_waves} boundary wavefronts first, halo exchange on a second stream while the interior is solved"
                                  if boundary_waves > 0 else "serial (no neighbours: nothing to overlap)"),
                     "serial_schedule_iterations_per_sec": serial_rate}
            if full:
                tot = tm["vertex_ms"] + tm["halo_ms"] + tm["edge_ms"] + tm["reduce_ms"]
                block["rank0_stage_share"] = {"vertex_step": tm["vertex_ms"] / tot, "halo_exchange": tm["halo_ms"] / tot,
                                              "edge_step": tm["edge_ms"] / tot, "all_reduce_and_control": tm["reduce_ms"] / tot,
                                              "source": "HIP events around every stage on the launch stream, replay of the window on rank 0"}
                block["rank0"] = {"V": part.graph.num_vertices, "E": part.graph.num_edges, "wavefronts": q["num_waves"],
                                  "newton_iterations_per_vertex": pcb2.inner_iters / max(part.graph.num_vertices - q["num_special"], 1)}
                if world > 1:      # the same lattice on one GPU, same loop: the strong-scaling reference
                    sdev = DeviceSolver(gl, "f32", device=local, columns="edge")
                    sel = time_window(sdev, pfirst, warmup, steps)
                    block["single_gpu_iterations_per_sec"] = steps / sel
                    block["speedup_vs_1gpu"] = sel / pel
                    sdev.close()
                try:
                    block["strip_model"] = strip_model(gl, local)
                except Exception as exc:
                    block["strip_model"] = {"error": f"{type(exc).__name__}: {exc}"}
            block["_rank0_partition"] = (part.graph, q, tm, pcb2)
    if watchdog is not None:
        watchdog.cancel()
    return block


def check_line(d):
    """The driver's contract for the printed line (keys, types, internal consistency): asserted by bench.py itself before it prints,
    by tests/test_bench_contract.py on a line produced in the test, and on the committed lines under profiles/."""
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(d[key], typ), key
    assert d["metric"] == "admm_iterations_per_sec" and d["unit"] == "iterations/s" and d["higher_is_better"] is True
    assert d["vs_baseline"] is None                      # BASELINE.md publishes no number for this metric
    assert "model" not in d["config"] and d["config"]["workload"] in ("benchmark4", "s10k", "s100k", "s6d")
    assert d["scaling"] in ("weak", "strong")
    per_step = d["n_gpus"] if d["scaling"] == "weak" else 1      # weak: N replicas each run K steps; strong: one graph, K steps
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - per_step) < 1e-6 * per_step, (d["value"], d["ms_per_step"])
    if d["n_gpus"] > 1:
        assert d["scaling"] == "strong" and d["config"]["workload"] == "s100k" and d["rccl_ranks"] == d["n_gpus"]
    r = d.get("roofline")
    if r is not None:
        assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] == HBM_PEAK_GBS
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and (r["traffic"] is None or r["traffic"] > 0)
        assert r["avg_launch_ms"] <= d["ms_per_step"] * (1 + 1e-9)          # a kernel's launch cannot outlast the step it is part of
    c = d.get("cpu_baseline")
    if c is not None:
        assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == d["unit"] and c["sample"]
        assert c["window"] == {k: d["config"]["window"][k] for k in ("first_iteration", "last_iteration")}      # like for like
    return True


def parse_args(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="benchmark4", choices=["benchmark4", "s10k", "s100k", "s6d"])
    ap.add_argument("--program", default="auto", choices=["auto", "wavefront", "workgroup"])
    ap.add_argument("--columns", default="auto", choices=["auto", "incidence", "edge"],
                    help="numbering of the state columns (include/gcsadmm.h edge_major_columns); auto = edge-major from 20 000 edges")
    ap.add_argument("--first", type=int, default=-1, help="ADMM iterations run untimed before the warm-up (default: benchmark4: the window is centred on "
                                                          "the run to the reference's stop; synthetic configs: a fixed start in the body of the run)")
    ap.add_argument("--cold-start", action="store_true", help="vertex solves from the fixed interior point every iteration (no warm start)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beyond the headline too: kernel shares and rooflines, the runs to the stop, the CPU oracle on the "
                         "same window, the configs.s10k / configs.s6d blocks and the sharded leg (at N > 1: the per-stage shares, the one-GPU "
                         "comparison, the strip model and the benchmark4 replicas)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: no CPU oracle")
    ap.add_argument("--no-configs", action="store_true", help="with --full, default workload only: skip the configs.s10k / configs.s6d blocks")
    ap.add_argument("--partition-timeout", type=int, default=240, help="seconds the sharded S100k leg may take at N > 1 before the line is printed without it")
    ap.add_argument("--loop-only", action="store_true",
                    help="with --full: only the timed loop and the per-kernel timing (no convergence runs, no CPU baseline): the "
                         "command to put under rocprofv3, so that its per-kernel averages cover the same launches as roofline.avg_launch_ms")
    ap.add_argument("--dry-launch", action="store_true", help="start the ranks and report what each one sees (RANK / WORLD_SIZE), no GPU work")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the timed loop computed in its last step as "
                                                          "DIR/<name>.npy (at N > 1 every rank its own strip, <name>_rank<r>.npy)")
    return ap.parse_args(argv)


def print_line(out):
    """check the contract, print the one JSON line"""
    try:      # the contract is asserted, but a violation must not cost the measurement: the line is printed with the finding in it
        check_line(out)
    except (AssertionError, KeyError) as exc:
        out["contract_violation"] = f"{type(exc).__name__}: {exc}"
    print(json.dumps(out), flush=True)
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args, argv)
    if args.dry_launch:
        return dry_launch(args)
    import numpy as np
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl")
    from gcs_admm_amd.solver import DeviceSolver

    if world > 1:
        return main_sharded(args, rank, world, local)

    g, dtype, extra = make_workload(args.workload)
    columns = args.columns if args.columns != "auto" else ("edge" if g.num_edges >= 20000 else "incidence")
    dev = DeviceSolver(g, dtype, device=local, program=args.program, columns=columns)
    if args.cold_start:
        _reset = dev.reset
        dev.reset = lambda **kw: _reset(cold_start=True, **kw)
    q = dev.query()
    program = "workgroup" if q["num_workgroup_vertices"] and not q["num_waves"] else ("wavefront" if not q["num_workgroup_vertices"] else "mixed")
    first = args.first if args.first >= 0 else window_start(args.workload, args.warmup, args.steps)
    el = time_window(dev, first, args.warmup, args.steps)
    cb = dev.read_control()
    assert cb.it == first + args.warmup + args.steps + 1, (cb.it, cb.status)
    its = args.steps / el
    if args.dump_outputs:
        dump_outputs(loop_outputs(dev, first, args.warmup, args.steps), args.dump_outputs)

    out = {"metric": "admm_iterations_per_sec", "value": its, "unit": "iterations/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * el / args.steps,
           "higher_is_better": True, "scaling": "weak",
           # the reference publishes no throughput number for this metric (`published` is {}); the rate derived from its
           # result record (solver time only, unknown hardware) is reported under reference_published, not as a baseline ratio
           "vs_baseline": None,
           "dtype": "f64" if dtype == "f64" else "f64 (interior point) on f32 state",
           "data": "synthetic" if args.workload != "benchmark4" else "fixture of the reference's test_data/benchmark4.py",
           "config": {"workload": args.workload, "V": g.num_vertices, "E": g.num_edges, "n": g.n,
                      "state_dtype": dtype, "state_columns": columns, "inner_arithmetic": "f64", "ipm_tol": IPM_TOL, "vertex_program": program,
                      "vertex_solves": "cold start every iteration" if args.cold_start else "warm start from the previous iteration's record (csrc/warm_start.h)",
                      "window": {"first_iteration": first + args.warmup + 1, "last_iteration": first + args.warmup + args.steps,
                                 "placement": ("centred on the run to the reference's stop (465 iterations)" if args.workload == "benchmark4" and args.first < 0
                                               else "fixed start in the body of the run"),
                                 "note": "the loop is advanced untimed from the zero state to the window (state preparation), then W warm-up and K timed "
                                         "iterations; the rate over the whole run is value_to_stop"},
                      "parallelism": "1 GPU",
                      "seed": None if args.workload == "benchmark4" else 0,
                      "degree_histogram": {int(k): int(v) for k, v in zip(*np.unique(np.diff(g.inc_ptr), return_counts=True))},
                      "facets_histogram": {int(k): int(v) for k, v in zip(*np.unique(np.diff(g.poly_ptr), return_counts=True))}}}
    if not args.full:      # a plain run: the headline only
        return print_line(out)
    sv, se, cb_, _ = kernel_shares(dev, first, args.warmup, min(args.steps, 200))
    out.update(rooflines(g, dtype, q, program, args.workload, out["ms_per_step"], sv, se, cb_, columns, with_flops=not args.loop_only))
    # ---- matched convergence: the reference's own stop rule ----
    if args.workload == "benchmark4" and not args.loop_only:
        dev.solve(chunk=100)                                                       # (untimed: the first whole solve of a process carries one-time costs of the host loop)
        runs = sorted((dev.solve(chunk=100) for _ in range(3)), key=lambda r: r["wall_time_s"])
        res = runs[1]                                                              # median of three whole runs
        gold = extra["case"]["golden_v3"]
        k = res["iterations"] + 1
        trace_ok = bool(res["iterations"] == gold["iterations"]
                        and np.allclose(res["pri_res_seq"][:k], gold["pri_res_seq"][:k], rtol=1e-3, atol=2e-4)
                        and np.allclose(res["dual_res_seq"][:k], gold["dual_res_seq"][:k], rtol=1e-3, atol=2e-4))
        timed = dev.solve(timed=True)
        out["value_to_stop"] = res["iterations"] / max(res["wall_time_s"], 1e-12)
        out["convergence"] = {"iterations_to_stop": res["iterations"], "reference_iterations": gold["iterations"],
                              "trace_within_reference_tolerance": trace_ok,
                              "cost": res["cost"], "reference_cost": gold["cost"],
                              "classic_cost": extra["case"]["golden_classic"]["cost"],
                              "loop_wall_time_s": res["wall_time_s"],
                              "iterations_per_sec_to_stop": out["value_to_stop"],
                              "runs": 3, "selection": "median wall time (after one untimed whole run)", "all_wall_times_s": [r["wall_time_s"] for r in runs],
                              "solve_time_s": timed["device_time_s"], "inner_failures": res["inner_failures"],
                              "window_rate_over_to_stop_rate": its / out["value_to_stop"],
                              "reference_solve_time_s": gold["solve_time"]}
        # iterations-to-eps (the second half of BASELINE.json's metric): eps_abs = eps_rel = 1e-6, MAX_IT lifted;
        # the relaxation optimum the monolithic solve reports (classic_solver record) is the yardstick
        tight = dev.solve(chunk=500, max_it=40000, eps_abs=1e-6, eps_rel=1e-6)
        classic = extra["case"]["golden_classic"]["cost"]
        out["iters_to_eps"] = {"eps_abs": 1e-6, "eps_rel": 1e-6, "iterations": tight["iterations"], "status": tight["status"],
                               "cost": tight["cost"], "rel_gap_to_classic": abs(tight["cost"] - classic) / classic,
                               "wall_time_s": tight["wall_time_s"], "iterations_per_sec": tight["iterations"] / max(tight["wall_time_s"], 1e-12)}
        out["reference_published"] = {"its_per_sec": REF_PUBLISHED_ITS, "ratio_of_this_run": its / REF_PUBLISHED_ITS,
                                      "note": "derived from the reference's committed record: 465 it / 37.88 s solver-time-only, hardware unknown "
                                              "(BASELINE.md section 1: not a published throughput number, hence vs_baseline = null)"}
    if args.workload == "s10k" and not args.loop_only:
        res = dev.solve(chunk=100)
        out["convergence"] = {"iterations_to_stop": res["iterations"], "status": res["status"], "cost": res["cost"],
                              "loop_wall_time_s": res["wall_time_s"], "inner_failures": res["inner_failures"],
                              "iterations_per_sec_to_stop": res["iterations"] / max(res["wall_time_s"], 1e-12),
                              "note": "f32 state; the f64 state and the CPU oracle stop at the same iteration (tests/test_gpu_configs.py)"}
    # ---- CPU baseline: the oracle on the host cores, the same iteration window, bounded sample ----
    if not args.no_cpu and not args.loop_only:
        try:
            out["cpu_baseline"] = cpu_baseline(g, args.workload, first, args.warmup, args.steps, seconds=15.0,
                                               dev=dev if g.num_vertices > 20000 else None, to_stop=args.workload == "benchmark4")
            out["gpu_over_cpu_same_window"] = its / out["cpu_baseline"]["value"]
            if "to_stop" in out["cpu_baseline"] and "value_to_stop" in out:
                out["gpu_over_cpu_to_stop"] = out["value_to_stop"] / out["cpu_baseline"]["to_stop"]["iterations_per_sec"]
        except Exception as exc:      # the checker's build or run failing must not cost the GPU measurement
            out["cpu_baseline"] = None
            out["cpu_baseline_error"] = f"{type(exc).__name__}: {exc}"
    # ---- the other single-GPU configs of BASELINE.json, compact (default line only) ----
    if args.workload == "benchmark4" and not args.loop_only and not args.no_configs:
        out["configs"] = {}
        for name, ks, kw in (("s10k", 100, 10), ("s6d", 10, 3)):
            try:
                out["configs"][name] = config_block(name, ks, kw, local, cpu=not args.no_cpu)
            except Exception as exc:      # the headline stands on its own
                out["configs"][name] = {"error": f"{type(exc).__name__}: {exc}"}
    # ---- the sharded path on one rank (same code, same RCCL calls as N > 1) ----
    if args.workload == "benchmark4" and not args.loop_only:
        try:
            blk = sharded_leg(args, 0, 1, local, min(args.steps, 100), min(args.warmup, 10), out, full=True)
            blk.pop("_rank0_partition", None)
        except Exception as exc:
            blk = {"error": f"{type(exc).__name__}: {exc}"}
        out["partitioned_s100k"] = blk
    return print_line(out)


def main_sharded(args, rank, world, local):
    """N > 1 ranks: the headline is the sharded path (BASELINE config 4, strong scaling); benchmark4 replicas are a side field (--full)"""
    import numpy as np
    import torch
    import torch.distributed as dist
    from gcs_admm_amd.solver import DeviceSolver
    out = {"metric": "admm_iterations_per_sec", "value": 0.0, "unit": "iterations/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": 0.0, "higher_is_better": True, "scaling": "strong",
           "vs_baseline": None, "dtype": "f64 (interior point) on f32 state", "data": "synthetic"}
    block = sharded_leg(args, rank, world, local, args.steps, args.warmup, out, full=args.full, dump=args.dump_outputs)
    rc = 0
    if rank == 0:
        if "error" in block:
            out["partitioned_s100k"] = block
            out["error"] = "the sharded leg failed: no N-GPU value"
            rc = 6
        else:
            pg, q, tm, pcb = block.pop("_rank0_partition")
            out["value"] = block["iterations_per_sec"]
            out["ms_per_step"] = block["ms_per_iteration"]
            out["rccl_ranks"] = block["rccl_ranks"]
            out["config"] = {"workload": "s100k", "V": block["V"], "E": block["E"], "n": 2, "state_dtype": "f32", "state_columns": "edge",
                             "inner_arithmetic": "f64", "ipm_tol": IPM_TOL, "vertex_program": "wavefront",
                             "window": block["window"], "parallelism": f"vertex partition: {world} row strips, one per GPU; RCCL halo exchange "
                                                                       "+ all-reduce of 6 f64 per iteration (gcsadmm_run_partitioned)", "seed": 0}
            if args.full:
                out["value_1gpu_same_workload"] = block.get("single_gpu_iterations_per_sec")
                out["speedup_vs_1gpu"] = block.get("speedup_vs_1gpu")
                # roofline of the dominant kernel on rank 0: its strip's algorithmic bytes per vertex-step launch over that launch's time
                tot = tm["vertex_ms"] + tm["halo_ms"] + tm["edge_ms"] + tm["reduce_ms"]
                v_ms = out["ms_per_step"] * tm["vertex_ms"] / tot
                alg = pg.algorithmic_bytes_per_iteration(4)
                ach = alg / (v_ms * 1e-3) / 1e9
                out["roofline"] = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": None,
                                   "kernel": "vertex_kernel<2> (rank 0's strip)", "avg_launch_ms": v_ms,
                                   "avg_launch_ms_source": "ms_per_step x the vertex step's share of rank 0's device time (HIP events around every stage, replay of the window)",
                                   "algorithmic_bytes_per_launch": alg, "waves": q["num_waves"],
                                   "note": "per-rank figure; the vertex step is bound by dependent f64 issue, not by HBM (DESIGN.md section 4)"}
            out["partitioned_s100k"] = block
    # ---- side field (--full): N independent replicas of benchmark4 (it does not shard) ----
    if args.full:
        try:
            g, dtype, _ = make_workload("benchmark4")
            dev = DeviceSolver(g, dtype, device=local)
            first = window_start("benchmark4", args.warmup, args.steps)
            el = time_window(dev, first, args.warmup, args.steps, barrier=dist.barrier)
            t = torch.tensor([el], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            if rank == 0:
                out["replicas_benchmark4"] = {"iterations_per_sec_all_replicas": args.steps / float(t.item()) * world, "replicas": world,
                                              "note": "throughput of N independent instances of the 42-vertex benchmark4 (no collective): not a scaling result"}
            dev.close()
        except Exception as exc:
            if rank == 0:
                out["replicas_benchmark4"] = {"error": f"{type(exc).__name__}: {exc}"}
    if rank == 0:
        if rc == 0:
            try:
                check_line(out)
            except (AssertionError, KeyError) as exc:
                out["contract_violation"] = f"{type(exc).__name__}: {exc}"
        print(json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main())
