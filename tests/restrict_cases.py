"""Cases, bounds and the host emulation for the path-restriction solve (csrc/path_restrict_core.h), shared by test_path_restrict.py
(CPU: the emulation) and test_gpu_path_restrict.py (gcsadmm_scene_restrict_paths).  A solver here is any callable
``solve(n, polys, paths, starts, tol, max_iter) -> (points per path, cost, iterations, status)`` on region INDICES.

Exact answers (boxes of half-width 0.6 on unit-spaced centres, the ends are regions): a corridor of k boxes along e_0 costs
(k - 1) - 1.2; a staircase of 2K + 1 boxes costs sqrt(2) (K - 1.2) and half of its segments have length zero; the elbow costs 1.6;
the all-zero case costs 0.  Bound on |cost - exact|: 2 deg tol + 1e-12 max(1, cost), deg = rows + segments -- the duality gap at the
stop (mu <= tol, gap = deg mu), counted twice."""
import ctypes as C
import os
import subprocess

import numpy as np

from gcs_admm_amd.graph import chebyshev_center, convert_pt_to_polytope
from gcs_admm_amd.rounding import solve_path_restriction

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gcs_admm_amd", "csrc")
SRC = os.path.join(HERE, "hostemu", "restrict_emu.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("path_restrict_core.h", "restrict_plan.h", "gcs_math.h", "step_args.h")] + \
       [os.path.join(ROOT, "include", "gcsadmm.h")]
LIB = os.path.join(HERE, "hostemu", "librestrictemu.so")
TOL, MAX_ITER = 1e-10, 100
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2
RECORDS = {"benchmark1": 3.236065, "benchmark2": 7.413745, "benchmark3": 60.177021, "benchmark4": 32.627198}


# ---- cases: (label, n, polys, path, exact cost or None) ----
def box(centre, half=0.6):
    c = np.asarray(centre, float)
    n = len(c)
    return np.vstack([np.eye(n), -np.eye(n)]), np.hstack([c + half, -(c - half)])


def _embed(c2, n):
    c = np.zeros(n); c[:min(n, 2)] = c2[:min(n, 2)]
    return c


def corridor(k, n):
    return f"corridor-k{k}-n{n}", n, [box(_embed([i, 0.0], n)) for i in range(k)], list(range(k)), (k - 1) - 1.2


def staircase(K):
    cen = [(0.0, 0.0)]
    for i in range(K):
        cen += [(i + 1.0, float(i)), (i + 1.0, i + 1.0)]
    return f"staircase-K{K}", 2, [box(c) for c in cen], list(range(2 * K + 1)), np.sqrt(2.0) * (K - 1.2)


ELBOW = [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (2.0, 1.0), (2.0, 2.0)]


def elbow(n=2):
    return f"elbow-n{n}", n, [box(_embed(c, n)) for c in ELBOW], list(range(5)), 1.6


def all_zero():
    return "all-zero", 2, [box(c) for c in [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)]], [0, 1, 2], 0.0


def exact_cases():
    out = [corridor(3, n) for n in (1, 2, 3, 8)] + [corridor(70, 2), corridor(130, 2)]
    return out + [staircase(K) for K in (3, 10, 35)] + [elbow(), all_zero()]


def with_point_terminals(case, analytic):
    """the case with 's' / 't' as points (convert_pt_to_polytope) at the centres of its first and last box; the analytic value holds
    up to 2 sqrt(n) 1e-6: the end points may move inside their boxes"""
    label, n, polys, path, _ = case
    s = 0.5 * (polys[0][1][:n] - polys[0][1][n:]); t = 0.5 * (polys[-1][1][:n] - polys[-1][1][n:])
    P = len(polys)
    return label + "-points", n, polys + [convert_pt_to_polytope(s), convert_pt_to_polytope(t)], [P] + path + [P + 1], analytic


def point_cases():
    """the corridor (straight line between the centres: k - 1) at n = 1, 2, 3, 8 and the elbow, which lives in a plane, at n = 2, 3, 8
    (round the corner (1.4, 0.6) of the third box: 2 sqrt(1.4^2 + 0.6^2))"""
    return [with_point_terminals(corridor(4, n), 3.0) for n in (1, 2, 3, 8)] + \
           [with_point_terminals(elbow(n), 2.0 * np.hypot(1.4, 0.6)) for n in (2, 3, 8)]


def mixed_rows_case():
    """n = 3: regions of 6 and 7 rows mixed (a box, or a box plus a redundant cut), on a bent chain"""
    cen = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1)]
    polys = []
    for i, c in enumerate(cen):
        A, b = box(np.array(c, float))
        if i % 2:
            a = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
            A = np.vstack([A, a]); b = np.hstack([b, a @ np.array(c, float) + 2.0])       # outside the box's corners (0.6 sqrt 3 = 1.04)
        polys.append((A, b))
    return "mixed-rows-n3", 3, polys, list(range(len(cen))), None


def benchmark_case(name, y_e=None):
    """the most probable path of a benchmark under the activations ``y_e`` (the oracle's run)"""
    from gcs_admm_amd.cases import fixture_sets
    from gcs_admm_amd.rounding import most_probable_path
    As, bs, n, _, _ = fixture_sets(name)
    keys = list(As)
    E = list(y_e)
    I_out = {v: [e for e in E if e[0] == v] for v in keys}
    path = most_probable_path(y_e, I_out)
    return name, n, [(np.asarray(As[v], float), np.asarray(bs[v], float)) for v in keys], [keys.index(v) for v in path], None


def oracle_activations(oracle_lib, name):
    """relaxed edge activations of a benchmark from the CPU oracle's run, as tests/test_rounding.py takes them"""
    from gcs_admm_amd import IPM_TOL
    from gcs_admm_amd.cases import load_fixture
    _, g = load_fixture(name)
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL)
    o.run(nthreads=4)
    E = g.edges_as_keys()
    return g.keys, E, {e: float(o.zedge[2 * g.n, i]) for i, e in enumerate(E)}


# ---- what the checks need ----
def point_rows(polys, path):
    """(A, b) of every point of the path: the rows of r_{j-1}, then those of r_j"""
    k = len(path)
    regs = [[path[0]]] + [[path[j - 1], path[j]] for j in range(1, k)] + [[path[-1]]]
    return [(np.vstack([polys[r][0] for r in reg]), np.hstack([polys[r][1] for r in reg])) for reg in regs]


def degree(polys, path):
    return sum(len(b) for _, b in point_rows(polys, path)) + len(path)


def bound(polys, path, cost, tol=TOL):
    return 2.0 * degree(polys, path) * tol + 1e-12 * max(1.0, abs(cost))


def host_start(polys, path):
    """Chebyshev centres of the one- or two-region intersections: the start of solve_path_restriction"""
    return np.array([chebyshev_center(A, b) for A, b in point_rows(polys, path)])


def host_cost(polys, path, n):
    cost, xs = solve_path_restriction({i: A for i, (A, _) in enumerate(polys)}, {i: b for i, (_, b) in enumerate(polys)}, n, path)
    assert xs is not None
    return cost


def assert_points_feasible(polys, path, pts):
    for (A, b), x in zip(point_rows(polys, path), pts):
        assert np.all(A @ x - b <= 1e-9 * np.maximum(1.0, np.abs(b))), (A @ x - b).max()


def assert_solution(case, pts, cost, its, st, reference=None, extra=0.0, max_iter=MAX_ITER):
    """the gates of one case: status, iteration limit, rows, and the cost against the exact answer (or ``reference``: the host's cost,
    which brings a bound of its own; ``extra``: what the analytic value of a point-terminal case is allowed on top)"""
    label, n, polys, path, exact = case
    print(f"{label}: cost {cost!r} exact {exact!r} host {reference!r} iterations {its} status {st} bound {bound(polys, path, cost):.3e}")
    assert st == 0, (label, st)
    assert 0 <= its <= max_iter, (label, its)
    assert np.isclose(cost, sum(np.linalg.norm(pts[j + 1] - pts[j]) for j in range(len(path))), rtol=1e-13, atol=1e-15), label
    assert_points_feasible(polys, path, pts)
    if exact is not None:
        assert abs(cost - exact) <= bound(polys, path, cost) + extra, (label, cost - exact)
    if reference is not None:
        assert abs(cost - reference) <= 2.0 * bound(polys, path, cost), (label, cost - reference)


# ---- CSR form of a call ----
def flatten(n, polys, paths, starts):
    """(poly_ptr, A, b, path_ptr, path_poly, start): the arrays of gcsadmm_scene_restrict_paths; path p's points at (path_ptr[p] + p) n"""
    ptr = np.zeros(len(polys) + 1, np.int32); ptr[1:] = np.cumsum([len(b) for _, b in polys])
    A = np.ascontiguousarray(np.vstack([np.asarray(a, float).reshape(-1, n) for a, _ in polys]))
    b = np.ascontiguousarray(np.hstack([np.asarray(v, float).ravel() for _, v in polys]))
    pp = np.zeros(len(paths) + 1, np.int32); pp[1:] = np.cumsum([len(p) for p in paths])
    poly = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32) for p in paths]) if paths else np.zeros(0, np.int32), np.int32)
    start = np.ascontiguousarray(np.concatenate([np.asarray(s, float).reshape(-1, n) for s in starts]) if starts else np.zeros((0, n)))
    assert start.shape[0] == int(pp[-1]) + len(paths)
    return ptr, A, b, pp, poly, start


def split_points(n, pp, flat):
    return [flat[int(pp[p]) + p:int(pp[p + 1]) + p + 1] for p in range(len(pp) - 1)]


# ---- the host emulation ----
def build_lib(out=LIB):
    if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in DEPS):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-O2", "-shared", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


_lib = None


def emu():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_lib())
        _lib.restrict_emu_error.restype = C.c_char_p
        _lib.restrict_emu_ws_doubles.restype = C.c_longlong
        _lib.restrict_emu_ws_doubles.argtypes = [C.c_int, C.c_longlong, C.c_longlong]
        _lib.restrict_emu_solve.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 4
        _lib.restrict_emu_plan.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    return _lib


def emu_raw(n, ptr, A, b, pp, poly, start, tol=TOL, max_iter=MAX_ITER, reverse=False):
    """restrict_emu_solve on the arrays: (return code, points, cost, iterations, status)"""
    num = len(pp) - 1
    pts = np.full_like(start, np.nan); cost = np.full(num, np.nan); its = np.full(num, -7, np.int32); st = np.full(num, -7, np.int32)
    rc = emu().restrict_emu_solve(n, len(ptr) - 1, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, num, pp.ctypes.data, poly.ctypes.data,
                                  start.ctypes.data, tol, max_iter, int(reverse), pts.ctypes.data, cost.ctypes.data, its.ctypes.data, st.ctypes.data)
    return rc, pts, cost, its, st


def emu_solver(reverse=False):
    def solve(n, polys, paths, starts, tol=TOL, max_iter=MAX_ITER):
        arrays = flatten(n, polys, paths, starts)
        rc, pts, cost, its, st = emu_raw(n, *arrays, tol=tol, max_iter=max_iter, reverse=reverse)
        assert rc == OK, emu().restrict_emu_error().decode()
        return split_points(n, arrays[3], pts), cost, its, st
    return solve


def device_solver(device=0):
    """gcsadmm_scene_restrict_paths through DeviceScene.restrict_paths, one scene per call"""
    from gcs_admm_amd.scene import DeviceScene

    def solve(n, polys, paths, starts, tol=TOL, max_iter=MAX_ITER):
        with DeviceScene(polys, device) as sc:
            return sc.restrict_paths(paths, starts, tol=tol, max_iter=max_iter)
    return solve
