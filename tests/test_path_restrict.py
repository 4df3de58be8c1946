"""The path-restriction solve without a GPU: gcs_admm_amd/csrc/path_restrict_core.h and restrict_plan.h compiled for the host
(tests/hostemu/restrict_emu.cpp: the tasks of every phase one after the other, forwards and backwards, unwritten workspace poisoned
with NaN).  Cases with exact answers, cases against the host solver (rounding.solve_path_restriction, the yardstick), the behaviour of
one call with many paths, the plan against a brute-force count, the rounding logic with the emulation injected as solver, and the
compiler's resource remarks of the kernels.  What the GPU computes is checked by test_gpu_path_restrict.py on the same cases.

What the body is held to: its exact cost within rc.bound (the duality gap at the stop, counted twice) on boxes at n = 1, 2, 3, 8 and on
general polytopes at every n = 1..8 -- rotated, translated up to 1e4 from the origin, rows of norm 1e-2 .. 1e2, up to 112 rows per
point, overlaps down to 1e-4, paths of 2 to 131 points with every count around a full chunk of the chain, 300 paths in one call
(restrict_cases.py lists the families).  The host solver, the yardstick of the cases without a closed form, is held to the closed
forms itself, within twice the bound.  Outside: centres 1e6 from the origin, overlaps thinner than 1e-4.  That these cases see errors
the boxes do not is shown by test_path_restrict_mutants.py."""
import functools

import numpy as np
import pytest

import restrict_cases as rc
from conftest import BENCHMARKS
from gcs_admm_amd import rounding as R
from gcs_admm_amd.cases import fixture_sets

ORDERS = [False, True]


@pytest.fixture(scope="module")
def activations(oracle_lib):
    """{benchmark: (V, E, y_e)} from the oracle's run, once for the module"""
    return {name: rc.oracle_activations(oracle_lib, name) for name in BENCHMARKS}


def solve_one(case, reverse=False, **kw):
    _, n, polys, path, _ = case
    pts, cost, its, st = rc.emu_solver(reverse)(n, polys, [path], [rc.case_start(case)], **kw)
    return pts[0], float(cost[0]), int(its[0]), int(st[0])


@pytest.mark.parametrize("reverse", ORDERS)
@pytest.mark.parametrize("case", rc.exact_cases(), ids=lambda c: c[0])
def test_exact_answers(case, reverse):
    rc.assert_solution(case, *solve_one(case, reverse))


@pytest.mark.parametrize("reverse", ORDERS)
@pytest.mark.parametrize("case", rc.point_cases() + [rc.mixed_rows_case()], ids=lambda c: c[0])
def test_against_the_host_solver(case, reverse):
    _, n, polys, path, _ = case
    extra = 2.0 * np.sqrt(n) * 1e-6 if case[4] is not None else 0.0
    rc.assert_solution(case, *solve_one(case, reverse), reference=rc.host_cost(polys, path, n), extra=extra)


# ---- general polytopes (restrict_cases.py: rotated, translated, rows of unequal norm, random facets, every n = 1..8) ----
@functools.lru_cache(maxsize=None)
def host_cost_of(label):
    _, n, polys, path, _ = next(c for c in rc.general_cases() if c[0] == label)
    return rc.host_cost(polys, path, n)


@pytest.mark.parametrize("reverse", ORDERS)
@pytest.mark.parametrize("case", rc.closed_form_cases(), ids=lambda c: c[0])
def test_closed_forms_on_general_polytopes(case, reverse):
    """families 1-6 and 8 against their exact costs, within the bound alone (no allowance for the end boxes: the exact value counts
    them in)"""
    rc.assert_solution(case, *solve_one(case, reverse))


HOST_POINTS = 34      # the host solver is dense: 1 to 13 s on the paths of 63 points and more, which it is no yardstick for here


@pytest.mark.parametrize("case", [c for c in rc.closed_form_cases() if len(c[3]) + 1 <= HOST_POINTS], ids=lambda c: c[0])
def test_host_solver_meets_the_closed_forms(case):
    """the yardstick of the cases without a closed form is itself held to the ones that have one"""
    label, n, polys, path, exact = case
    cost = host_cost_of(label)
    print(f"{label}: host {cost!r} exact {exact!r} bound {rc.bound(polys, path, cost):.3e}")
    assert abs(cost - exact) <= 2.0 * rc.bound(polys, path, cost), (label, cost - exact)


@pytest.mark.parametrize("reverse", ORDERS)
@pytest.mark.parametrize("case", rc.family("bent"), ids=lambda c: c[0])
def test_bent_chains_against_the_host_solver(case, reverse):
    rc.assert_solution(case, *solve_one(case, reverse), reference=host_cost_of(case[0]))


def test_thin_overlaps_leave_headroom():
    """the thinnest overlap that is tested (1e-4) is one the method reaches with a fifth of the iteration limit to spare"""
    for case in rc.family("thin"):
        _, _, its, st = solve_one(case)
        assert st == 0 and its <= 0.8 * rc.MAX_ITER, (case[0], its)


def test_task_order_does_not_matter_on_general_polytopes():
    for case in rc.general_cases():
        (_, c0, i0, s0), (_, c1, i1, s1) = solve_one(case, False), solve_one(case, True)
        assert s0 == s1 == 0 and abs(i0 - i1) <= 1 and abs(c0 - c1) <= rc.bound(case[2], case[3], c0), case[0]


@functools.lru_cache(maxsize=None)
def wide_call():
    return rc.wide_call()


def check_wide_call(solve):
    """300 paths of 2 to 41 points in one call (more workgroups than the device has compute units): every one converges to its exact
    cost, and eight of them, the shortest and the longest among them, come out bit for bit as they do alone"""
    n, polys, paths, starts, exact = wide_call()
    assert len(paths) == rc.WIDE_PATHS and len(paths[0]) == 1 and len(paths[-1]) == rc.WIDE_CHAIN
    pts, cost, its, st = solve(n, polys, paths, starts)
    assert not np.any(st), list(np.nonzero(st)[0])
    worst = 0.0
    for p, path in enumerate(paths):
        rc.assert_points_feasible(polys, path, pts[p])
        bnd = rc.bound(polys, path, cost[p])
        worst = max(worst, abs(cost[p] - exact[p]) / bnd)
        assert abs(cost[p] - exact[p]) <= bnd, (p, len(path), cost[p] - exact[p])
    print(f"wide call: worst |cost - exact| / bound {worst:.3f}")
    for p in rc.WIDE_SOLO:
        solo_pts, solo_cost, solo_its, solo_st = solve(n, polys, [paths[p]], [starts[p]])
        assert solo_st[0] == 0 and solo_its[0] == its[p], p
        assert solo_cost[0] == cost[p] and np.array_equal(solo_pts[0], pts[p]), p            # bit for bit
    return worst


def test_wide_call():
    check_wide_call(rc.emu_solver())


@pytest.mark.parametrize("name", BENCHMARKS)
def test_most_probable_paths_of_the_benchmarks(activations, name):
    case = rc.benchmark_case(name, activations[name][2])
    _, n, polys, path, _ = case
    ref = rc.host_cost(polys, path, n)
    for reverse in ORDERS:
        rc.assert_solution(case, *solve_one(case, reverse), reference=ref)


def test_task_order_does_not_matter():
    """forwards and backwards agree within the bound, iteration counts within one"""
    for case in rc.exact_cases() + [rc.mixed_rows_case()]:
        (_, c0, i0, s0), (_, c1, i1, s1) = solve_one(case, False), solve_one(case, True)
        assert s0 == s1 == 0 and abs(i0 - i1) <= 1 and abs(c0 - c1) <= rc.bound(case[2], case[3], c0), case[0]


def mixed_call():
    """one scene (a corridor of 130 boxes and three boxes at 0, 1, 5 on a second row) and paths of 3, 7, 71 and 131 points, plus one
    whose middle regions are disjoint"""
    _, n, polys, _, _ = rc.corridor(130, 2)
    far = len(polys)
    polys = polys + [rc.box([0.0, 3.0]), rc.box([1.0, 3.0]), rc.box([5.0, 3.0])]
    paths = [list(range(2)), list(range(10, 16)), list(range(30, 100)), list(range(130)), [far, far + 1, far + 2]]
    starts = [rc.host_start(polys, p) for p in paths[:4]]
    cen = np.array([[0.0, 3.0], [0.5, 3.0], [3.0, 3.0], [5.0, 3.0]])      # (the third point would have to lie in boxes 1 and 5)
    return n, polys, paths, starts + [cen]


def check_mixed_call(solve):
    n, polys, paths, starts = mixed_call()
    assert [len(p) + 1 for p in paths[:4]] == [3, 7, 71, 131]
    pts, cost, its, st = solve(n, polys, paths, starts)
    assert list(st) == [0, 0, 0, 0, 1] and np.isinf(cost[4]) and np.all(np.isfinite(cost[:4]))
    for p in range(4):
        solo_pts, solo_cost, solo_its, solo_st = solve(n, polys, [paths[p]], [starts[p]])
        assert solo_st[0] == 0 and solo_its[0] == its[p]
        assert solo_cost[0] == cost[p] and np.array_equal(solo_pts[0], pts[p]), p           # bit for bit
        assert abs(cost[p] - max(0.0, (len(paths[p]) - 1) - 1.2)) <= rc.bound(polys, paths[p], cost[p])      # (two boxes overlap: 0)
    without, cost4, _, st4 = solve(n, polys, paths[:4], starts[:4])
    assert np.array_equal(cost4, cost[:4]) and list(st4) == [0, 0, 0, 0]


@pytest.mark.parametrize("reverse", ORDERS)
def test_paths_of_one_call_do_not_affect_each_other(reverse):
    check_mixed_call(rc.emu_solver(reverse))


def test_iteration_limit_is_a_failure():
    pts, cost, its, st = solve_one(rc.staircase(3), max_iter=3)
    assert st == -1 and its == 3 and np.isinf(cost) and np.all(np.isfinite(pts))


def test_bad_arguments():
    n, polys, paths, starts = mixed_call()
    arrays = list(rc.flatten(n, polys, paths[:2], starts[:2]))
    for bad in (len(polys), -1):
        a = [x.copy() for x in arrays]
        a[4][3] = bad
        rcode, *_ = rc.emu_raw(n, *a)
        assert rcode == rc.BAD_ARG and "out of range" in rc.emu().restrict_emu_error().decode()
    a = [x.copy() for x in arrays]
    a[3][:] = [0, 0, len(a[4])]                               # an empty first path
    rcode, *_ = rc.emu_raw(n, *a)
    assert rcode == rc.BAD_ARG and "at least one region" in rc.emu().restrict_emu_error().decode()


def run_plan(n, ptr, pp, poly, want_arrays=True):
    num = len(pp) - 1
    totals = np.zeros(6, np.int64)
    prefix = np.full(int(pp[-1]) + 2 * num, -1, np.int32) if want_arrays else None
    ws_off = np.full(num, -1, np.int64) if want_arrays else None
    code = rc.emu().restrict_emu_plan(n, len(ptr) - 1, ptr.ctypes.data, num, pp.ctypes.data, poly.ctypes.data, totals.ctypes.data,
                                      prefix.ctypes.data if want_arrays else None, ws_off.ctypes.data if want_arrays else None)
    return code, totals, prefix, ws_off


@pytest.mark.parametrize("n", [1, 2, 6, 8])
def test_plan_against_a_brute_force_count(n):
    """offsets and sizes of restrict_plan.h: the row prefix by listing every (point, row) pair, the workspace by listing every array
    the solve keeps (path_restrict_core.h), 32-double slabs, one workgroup of 64 lanes per path"""
    rng = np.random.default_rng(n)
    rows = rng.integers(1, 9, 12)
    ptr = np.zeros(13, np.int32); ptr[1:] = np.cumsum(rows)
    paths = [list(rng.integers(0, 12, k)) for k in (1, 2, 5, 40, 3)]
    pp = np.zeros(len(paths) + 1, np.int32); pp[1:] = np.cumsum([len(p) for p in paths])
    poly = np.concatenate(paths).astype(np.int32)
    code, totals, prefix, ws_off = run_plan(n, ptr, pp, poly)
    assert code == rc.OK
    at, all_rows, Q = 0, 0, n + 1
    for p, path in enumerate(paths):
        k = len(path)
        pairs = [(j, r) for j in range(k + 1) for reg in ([path[j - 1]] if j >= 1 else []) + ([path[j]] if j < k else []) for r in range(rows[reg])]
        want = [sum(1 for j, _ in pairs if j < jj) for jj in range(k + 2)]
        off = int(pp[p]) + 2 * p
        assert list(prefix[off:off + k + 2]) == want and want[-1] == len(pairs)
        assert ws_off[p] == at and at % 32 == 0
        Rp = len(pairs)
        doubles = (n * (k + 1) + k) + 6 * Rp + k * (7 * Q + 1) + Q * Q * (k + 1) + Q * Q * k + Q * (k + 1)      # q, t | rows | cones | blocks | dw
        assert rc.emu().restrict_emu_ws_doubles(n, k, Rp) == doubles
        at += -(-doubles // 32) * 32
        all_rows += Rp
    assert list(totals) == [len(paths), 64, int(pp[-1]), int(pp[-1]) + len(paths), all_rows, at]


def test_plan_refuses_totals_that_do_not_fit():
    """before anything is allocated: the plan alone decides (no array of that size exists here either)"""
    ptr = np.array([0, 1 << 30], np.int32)                      # one region with 2^30 rows
    pp = np.array([0, 2], np.int32); poly = np.zeros(2, np.int32)
    code, *_ = run_plan(2, ptr, pp, poly, want_arrays=False)      # 4 2^30 rows on the path
    assert code == rc.UNSUPPORTED and "2^31 - 1 rows" in rc.emu().restrict_emu_error().decode()
    code, *_ = run_plan(9, np.array([0, 4], np.int32), pp, poly, want_arrays=False)
    assert code == rc.UNSUPPORTED


# ---- the rounding logic with the emulation injected ----
def host_centres(polys):
    from gcs_admm_amd.graph import chebyshev_center
    cen, rad = [], []
    for A, b in polys:
        try:
            c = chebyshev_center(A, b)
            cen.append(c); rad.append(float(np.min((b - A @ c) / np.linalg.norm(A, axis=1))))
        except ValueError:
            cen.append(np.zeros(A.shape[1])); rad.append(-1.0)
    return np.array(cen), np.array(rad), np.zeros(len(polys), np.int32)


def emu_restrict(polys, paths, starts):
    return rc.emu_solver()(np.asarray(polys[0][0]).shape[1], polys, paths, starts)


EMU_SOLVER = functools.partial(R.solve_path_restrictions, centers=host_centres, restrict=emu_restrict)


def path_bound(As, path):
    return 2.0 * (sum(2 * len(As[v]) for v in path) + len(path)) * rc.TOL


@pytest.mark.parametrize("name", BENCHMARKS)
def test_rounding_with_the_emulation_as_solver(activations, monkeypatch, name):
    """seeds 0-4: the device branch visits the host's candidate list, meets the reference's record and the host's result"""
    As, bs, n, _, _ = fixture_sets(name)
    V, E, y_e = activations[name]
    I_out = {v: [e for e in E if e[0] == v] for v in V}
    host_solve = R.solve_path_restriction
    for seed in range(5):
        visited_host, visited_dev = [], []

        def spy_host(As_, bs_, n_, path):
            visited_host.append(tuple(path))
            return host_solve(As_, bs_, n_, path)

        def spy_dev(As_, bs_, n_, paths):
            visited_dev.extend(tuple(p) for p in paths)
            return EMU_SOLVER(As_, bs_, n_, paths)
        monkeypatch.setattr(R, "solve_path_restriction", spy_host)
        cost_h, xv_h, yv_h = R.rounding(y_e, V, E, I_out, As, bs, n, seed=seed)
        monkeypatch.setattr(R, "solve_path_restriction", host_solve)
        cost_d, xv_d, yv_d = R.rounding(y_e, V, E, I_out, As, bs, n, seed=seed, restriction="device", solver=spy_dev)
        print(f"{name} seed {seed}: host {cost_h!r} emulation {cost_d!r} candidates {len(visited_dev)}")
        assert visited_dev == visited_host and len(visited_dev) >= 1
        assert abs(cost_d - rc.RECORDS[name]) <= 1e-5 * rc.RECORDS[name]
        bnd = max(path_bound(As, p) for p in visited_dev) + 1e-12 * max(1.0, cost_d)
        assert abs(cost_d - cost_h) <= 2.0 * bnd
        assert set(xv_d) == set(V) and yv_d['s'] == 1 and yv_d['t'] == 1
        for v in V:
            if yv_d[v]:
                for half in (xv_d[v][:n], xv_d[v][n:]):
                    assert np.all(As[v] @ half <= bs[v] + 1e-9 * np.maximum(1.0, np.abs(bs[v])))


def test_infeasible_candidates_keep_the_draws_going(activations, monkeypatch):
    """a solver that calls the most probable path infeasible: the device branch solves N paths in its first call, goes on with the
    remaining draws, and has visited what the host loop visits with the same rejection"""
    name = "benchmark4"
    As, bs, n, _, _ = fixture_sets(name)
    V, E, y_e = activations[name]
    I_out = {v: [e for e in E if e[0] == v] for v in V}
    first = tuple(R.most_probable_path(y_e, I_out))
    seen_dev, seen_host, rounds = [], [], []
    host_solve = R.solve_path_restriction

    def picky(As_, bs_, n_, paths):
        rounds.append(len(paths)); seen_dev.extend(tuple(p) for p in paths)
        return [(float('inf'), None) if tuple(p) == first else r for p, r in zip(paths, EMU_SOLVER(As_, bs_, n_, paths))]

    def picky_host(As_, bs_, n_, path):
        seen_host.append(tuple(path))
        return (float('inf'), None) if tuple(path) == first else host_solve(As_, bs_, n_, path)
    cost, xv, yv = R.rounding(y_e, V, E, I_out, As, bs, n, N=3, seed=1, restriction="device", solver=picky)
    monkeypatch.setattr(R, "solve_path_restriction", picky_host)
    cost_h, _, _ = R.rounding(y_e, V, E, I_out, As, bs, n, N=3, seed=1)
    assert rounds[0] == 3 and len(rounds) >= 2 and sum(rounds) == 4, rounds
    assert seen_dev == seen_host and seen_dev[0] == first
    assert np.isfinite(cost) and abs(cost - cost_h) <= 1e-6


def test_rounding_many_equals_rounding_alone(activations):
    """eight copies of benchmark4 with different seeds through one solver call per round: per copy what rounding returns alone"""
    name = "benchmark4"
    As, bs, n, _, _ = fixture_sets(name)
    V, E, y_e = activations[name]
    I_out = {v: [e for e in E if e[0] == v] for v in V}
    calls = []

    def counting(As_, bs_, n_, paths):
        calls.append(len(paths))
        return EMU_SOLVER(As_, bs_, n_, paths)
    problems = [dict(y_e_sol=y_e, V=V, E=E, I_v_out=I_out, As=As, bs=bs, n=n, seed=seed) for seed in range(8)]
    many = R.rounding_many(problems, solver=counting)
    assert calls[0] >= 8 and len(calls) <= 20
    for seed, (cost, xv, yv) in enumerate(many):
        c1, x1, y1 = R.rounding(y_e, V, E, I_out, As, bs, n, seed=seed, restriction="device", solver=EMU_SOLVER)
        assert cost == c1 and yv == y1 and all(np.array_equal(xv[v], x1[v]) for v in V), seed


def test_default_restriction_is_the_host(activations):
    name = "benchmark1"
    As, bs, n, _, _ = fixture_sets(name)
    V, E, y_e = activations[name]
    I_out = {v: [e for e in E if e[0] == v] for v in V}

    def never(*a):
        raise AssertionError("the default must not call the device solver")
    cost, _, _ = R.rounding(y_e, V, E, I_out, As, bs, n, solver=never)
    assert abs(cost - rc.RECORDS[name]) <= 1e-5 * rc.RECORDS[name]
    with pytest.raises(ValueError):
        R.rounding(y_e, V, E, I_out, As, bs, n, restriction="gpu")


def test_kernels_use_no_scratch():
    """the compiler's resource remarks: every instantiation n = 1..8 of the path kernel is there, without scratch"""
    from gcs_admm_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if "path_restrict_kernel" in k}
    assert len(res) == 8, sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)
        assert r["lds"] <= 64 * 1024, (name, r)


def test_cli_has_the_rounding_switch():
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(rc.ROOT, "admm_solver_v3.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--rounding {host,device}" in r.stdout
