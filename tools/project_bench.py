"""Measurement for the nearest regions of points outside the cover (``DeviceScene.project``: project_list_kernel and project_solve_kernel,
csrc/point_project_core.h): seconds per ``project`` call -- upload of the points, count pass, scan on the host, fill pass, one solve per
candidate, read-back of the seven arrays -- on lattices of 1 000 and 20 000 overlapping cells in R^2, for Q = 1, 8, 64 points placed
0.01 to 0.5 outside the cover, each with the default radius of ``SceneQueries.nearest_regions`` (the distance to the nearest Chebyshev
centre).  Medians of ``--reps`` calls after a warm-up call, with the spread; every time is a host clock around a call that ends in a copy
from the device.  Per line also the candidates, the solves that took a step, the iterations per solve, the statuses, and the same pairs
through the host fallback (``scipy.optimize.minimize(method="SLSQP")``, at most ``--host-pairs`` of them) as a yardstick, with the
largest difference between its distances and the device's.  One JSON line per (lattice, Q).

  python tools/project_bench.py [--regions 1000 20000] [--points 1 8 64] [--reps 7] [--host-pairs 200]
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401  (HIP runtime first, see abi.load_library)
from scipy.optimize import minimize
from gcs_admm_amd.scene import DeviceScene


def lattice(P):
    """(polys, nx, ny): nx x ny cells [i - 0.05, i + 1.05] x [j - 0.05, j + 1.05], nx ny >= P cut to P"""
    ny = max(int(np.sqrt(P / 2)), 1)
    nx = -(-P // ny)
    A = np.vstack([np.eye(2), -np.eye(2)])
    polys = [(A, np.array([i + 1.05, j + 1.05, -(i - 0.05), -(j - 0.05)])) for i in range(nx) for j in range(ny)][:P]
    return polys, nx, ny


def outside_points(rng, Q, ny):
    """Q points 0.01 to 0.5 to the left of the cover (the first column of cells is complete whatever P is)"""
    return np.column_stack([-0.05 - rng.uniform(0.01, 0.5, Q), rng.uniform(0.0, ny, Q)])


def host_projection(A, b, c, p):
    res = minimize(lambda x: 0.5 * float((x - p) @ (x - p)), c, jac=lambda x: x - p, method="SLSQP",
                   constraints=[dict(type="ineq", fun=lambda x: b - A @ x, jac=lambda x: -A)], options=dict(ftol=1e-15, maxiter=200))
    return res.x


def measure(P, counts, reps, host_pairs):
    polys, nx, ny = lattice(P)
    rng = np.random.default_rng(P)
    clock = time.perf_counter
    with DeviceScene(polys) as scene:
        centers = scene.centers()[0]
        for Q in counts:
            pts = outside_points(rng, Q, ny)
            rad = np.array([np.sqrt(((centers - p) ** 2).sum(axis=1)).min() for p in pts])
            scene.project(pts, rad)                                      # warm-up at this shape
            t = []
            for _ in range(reps):
                t0 = clock(); res = scene.project(pts, rad); t.append(clock() - t0)
            hit_ptr, region, cls, dist, near, status, its = res
            point_of = np.repeat(np.arange(Q), np.diff(hit_ptr))
            take = np.arange(len(region))[:host_pairs]
            t0 = clock()
            host = np.array([np.linalg.norm(host_projection(*polys[region[k]], centers[region[k]], pts[point_of[k]]) - pts[point_of[k]]) for k in take])
            t_host = clock() - t0
            solved = status >= 0
            print(json.dumps({"metric": "seconds_per_project_call", "n": 2, "regions": P, "points": Q, "repeats": reps,
                              "project_call_s": float(np.median(t)), "project_call_s_spread": [float(min(t)), float(max(t))],
                              "candidates": int(len(region)), "candidates_per_point": len(region) / Q, "solves": int((cls == 2).sum()),
                              "iterations_per_solve": float(its[cls == 2].mean()) if np.any(cls == 2) else 0.0, "iterations_max": int(its.max()) if len(its) else 0,
                              "status_solved": int((status == 0).sum()), "status_beyond": int((status == 1).sum()), "status_failed": int((status < 0).sum()),
                              "nearest_distance_mean": float(np.mean([dist[hit_ptr[q]:hit_ptr[q + 1]][status[hit_ptr[q]:hit_ptr[q + 1]] == 0].min() for q in range(Q)])),
                              "host_pairs": int(len(take)), "host_s_per_pair": t_host / max(len(take), 1),
                              "device_s_per_candidate": float(np.median(t)) / max(len(region), 1),
                              "host_device_distance_diff_max": float(np.abs(host - dist[take])[solved[take]].max()) if np.any(solved[take]) else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, nargs="*", default=[1000, 20000])
    ap.add_argument("--points", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-pairs", type=int, default=200)
    args = ap.parse_args()
    for P in args.regions:
        measure(P, args.points, args.reps, args.host_pairs)


if __name__ == "__main__":
    main()
