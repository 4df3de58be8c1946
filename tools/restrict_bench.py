#!/usr/bin/env python3
"""Rounding step: the host restriction (rounding.solve_path_restriction, unchanged) against the device call
(DeviceScene.restrict_paths = gcsadmm_scene_restrict_paths) on corridors and staircases of unit boxes.

    python tools/restrict_bench.py [--k 25 100 400] [--reps 5] [--host-max-k 400] [--out FILE.json]

Per shape and k: one path solved by the host (wall time of one call), 5 and 64 x 5 copies of it solved by one device call (host clock
around the call, which ends in a synchronise: uploads, allocation, launch and downloads included), medians of --reps repetitions after
one warm-up each, the two sides alternating inside a repetition.  The costs must agree within the duality-gap bound of both solvers in
every line, or the script fails.  Then, at n = 2 and n = 6 (corridors), the device time per Newton iteration, taken as the difference of
a full call and a call with max_iter = 0 (which does everything but iterate) over the iteration count, and its slope over k: the time of
one block of one iteration -- one step of the factorisation, two forward and two backward substitution steps of the chain on lane 0,
plus that block's share of the lane-parallel phases.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcs_admm_amd.rounding import solve_path_restriction  # noqa: E402
from gcs_admm_amd.scene import DeviceScene  # noqa: E402

TOL = 1e-10


def box(c, half=0.6):
    c = np.asarray(c, float)
    n = len(c)
    return np.vstack([np.eye(n), -np.eye(n)]), np.hstack([c + half, -(c - half)])


def corridor(k, n=2):
    return [box([float(i)] + [0.0] * (n - 1)) for i in range(k)], (k - 1) - 1.2


def staircase(k):
    K = (k - 1) // 2
    cen = [(0.0, 0.0)]
    for i in range(K):
        cen += [(i + 1.0, float(i)), (i + 1.0, i + 1.0)]
    return [box(c) for c in cen], np.sqrt(2.0) * (K - 1.2)


def start_of(polys):
    """Chebyshev centres of the intersections along the whole chain (boxes: the midpoints of the overlaps)"""
    lo = [-(b[len(b) // 2:]) for _, b in polys]; hi = [b[:len(b) // 2] for _, b in polys]
    k = len(polys)
    pts = [0.5 * (lo[0] + hi[0])]
    pts += [0.5 * (np.maximum(lo[j - 1], lo[j]) + np.minimum(hi[j - 1], hi[j])) for j in range(1, k)]
    return np.array(pts + [0.5 * (lo[-1] + hi[-1])])


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[25, 100, 400])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max-k", type=int, default=400, help="largest k the host solver is timed at")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for shape, make in (("corridor", corridor), ("staircase", staircase)):
        for k in args.k:
            polys, exact = make(k)
            kk, n = len(polys), 2
            path = list(range(kk))
            As = {i: A for i, (A, _) in enumerate(polys)}; bs = {i: b for i, (_, b) in enumerate(polys)}
            x0 = start_of(polys)
            deg = sum(2 * len(b) for _, b in polys) + kk
            with DeviceScene(polys) as sc:
                dev = {copies: (lambda c=copies: sc.restrict_paths([path] * c, [x0] * c, tol=TOL)) for copies in (5, 320)}
                host = (lambda: solve_path_restriction(As, bs, n, path)) if kk <= args.host_max_k else None
                for f in dev.values():
                    f()                                                     # warm-up
                if host:
                    host()
                t = {"host": [], 5: [], 320: []}
                cost_h, cost_d, iters = None, None, None
                for _ in range(args.reps):                                  # the sides alternate inside a repetition
                    if host:
                        dt, (cost_h, _) = timed(host); t["host"].append(dt)
                    for copies, f in dev.items():
                        dt, (_, cost, its, st) = timed(f); t[copies].append(dt)
                        assert np.all(st == 0) and np.all(cost == cost[0]), (shape, k, st)
                        cost_d, iters = float(cost[0]), int(its[0])
                bound = 2.0 * deg * TOL + 1e-12 * max(1.0, cost_d)
                assert abs(cost_d - exact) <= bound, (shape, k, cost_d, exact)
                if host:
                    assert abs(cost_d - cost_h) <= 2.0 * bound, (shape, k, cost_d, cost_h)
                med = {key: (statistics.median(v) if v else None) for key, v in t.items()}
                emit(kind="compare", shape=shape, regions=kk, n=n, exact=exact, cost_device=cost_d, cost_host=cost_h, newton_iterations=iters,
                     host_s_per_path=med["host"], device_s_5_paths=med[5], device_s_320_paths=med[320],
                     host_s_5_paths=None if med["host"] is None else 5 * med["host"],
                     host_over_device_5_paths=None if med["host"] is None else 5 * med["host"] / med[5],
                     host_over_device_320_paths=None if med["host"] is None else 320 * med["host"] / med[320],
                     spread_5=[min(t[5]), max(t[5])], spread_320=[min(t[320]), max(t[320])], reps=args.reps)
    for n in (2, 6):
        per_iter = {}
        for k in args.k:
            polys, exact = corridor(k, n)
            path, x0 = list(range(k)), start_of(polys)
            with DeviceScene(polys) as sc:
                full = lambda: sc.restrict_paths([path], [x0], tol=TOL)
                none = lambda: sc.restrict_paths([path], [x0], tol=TOL, max_iter=0)
                full(); none()
                tf, tn, its = [], [], None
                for _ in range(args.reps):
                    dt, (_, cost, it, st) = timed(full); tf.append(dt)
                    assert st[0] == 0 and abs(cost[0] - exact) <= 2.0 * (2 * k * 2 * n + k) * TOL + 1e-12 * max(1.0, exact)
                    its = int(it[0])
                    dt, _ = timed(none); tn.append(dt)
                per_iter[k] = (statistics.median(tf) - statistics.median(tn)) / its
                emit(kind="newton", n=n, regions=k, newton_iterations=its, call_s=statistics.median(tf), call_without_iterations_s=statistics.median(tn),
                     device_s_per_newton_iteration=per_iter[k])
        ks = sorted(per_iter)
        if len(ks) >= 2:
            emit(kind="block", n=n, from_regions=ks[0], to_regions=ks[-1],
                 device_s_per_block_of_one_iteration=(per_iter[ks[-1]] - per_iter[ks[0]]) / (ks[-1] - ks[0]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
