"""gcsadmm_scene_restrict_paths on the MI355X: the cases of test_path_restrict.py (exact answers, the host solver as yardstick, one call
with many paths, refused arguments) through the C ABI, the device against the host emulation of the same body, and the rounding step
with ``restriction="device"`` up to the command line.

Every instantiation n = 1..8 of path_restrict_kernel is launched on regions that are no boxes (restrict_cases.py: rotated, translated,
rows of unequal norm, random facets, up to 112 rows per point on 64 lanes, 31 .. 97 points around the chunks of the chain, a path of
one region, 300 paths in one launch), each cost within rc.bound of its closed form and of nothing wider; the bent chains, which have
none, within twice the bound of the host solver.  Outside the contract: centres 1e6 from the origin, overlaps thinner than 1e-4.

Measured on an MI355X, worst |cost - exact| / bound per family (bent: |cost - host| / (2 bound)); the emulation gave the same
figures to the digits shown, and the same iteration counts:
  moved 0.069   line 0.038   thin 0.017   far 0.024   reflection 0.070   intervals 0.048   bent 0.290   single 0   wide call 0.013"""
import os
import subprocess
import sys

import numpy as np
import pytest

import restrict_cases as rc
from conftest import BENCHMARKS
from gcs_admm_amd import rounding as R
from gcs_admm_amd.cases import fixture_sets, load_fixture
from test_path_restrict import check_mixed_call, check_wide_call, mixed_call, path_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def activations(oracle_lib):
    return {name: rc.oracle_activations(oracle_lib, name) for name in BENCHMARKS}


def solve_one(case, solver):
    _, n, polys, path, _ = case
    pts, cost, its, st = solver(n, polys, [path], [rc.case_start(case)])
    return pts[0], float(cost[0]), int(its[0]), int(st[0])


@pytest.mark.parametrize("case", rc.exact_cases(), ids=lambda c: c[0])
def test_exact_answers(case):
    rc.assert_solution(case, *solve_one(case, rc.device_solver()))


@pytest.mark.parametrize("case", rc.point_cases() + [rc.mixed_rows_case()], ids=lambda c: c[0])
def test_against_the_host_solver(case):
    _, n, polys, path, _ = case
    extra = 2.0 * np.sqrt(n) * 1e-6 if case[4] is not None else 0.0
    rc.assert_solution(case, *solve_one(case, rc.device_solver()), reference=rc.host_cost(polys, path, n), extra=extra)


@pytest.mark.parametrize("name", BENCHMARKS)
def test_most_probable_paths_of_the_benchmarks(activations, name):
    case = rc.benchmark_case(name, activations[name][2])
    _, n, polys, path, _ = case
    rc.assert_solution(case, *solve_one(case, rc.device_solver()), reference=rc.host_cost(polys, path, n))


_device = {}


def device_result(case):
    """what the device returns for a general-polytope case, solved once per label"""
    if case[0] not in _device:
        _device[case[0]] = solve_one(case, rc.device_solver())
    return _device[case[0]]


@pytest.mark.parametrize("case", rc.closed_form_cases(), ids=lambda c: c[0])
def test_closed_forms_on_general_polytopes(case):
    """families 1-6 and 8: every instantiation n = 1..8 on regions that are no boxes, within the bound alone"""
    rc.assert_solution(case, *device_result(case))


@pytest.mark.parametrize("case", rc.family("bent"), ids=lambda c: c[0])
def test_bent_chains_against_the_host_solver(case):
    _, n, polys, path, _ = case
    rc.assert_solution(case, *device_result(case), reference=rc.host_cost(polys, path, n))


def test_device_and_emulation_agree():
    """the same body on the device and on the host: status equal, costs within the bound, iteration counts within one"""
    dev, emu = rc.device_solver(), rc.emu_solver()
    for case in rc.exact_cases() + rc.point_cases() + [rc.mixed_rows_case()]:
        (_, cd, itd, sd), (_, ce, ite, se) = solve_one(case, dev), solve_one(case, emu)
        print(f"{case[0]}: device {cd!r} ({itd}) emulation {ce!r} ({ite})")
        assert sd == se == 0 and abs(itd - ite) <= 1 and abs(cd - ce) <= rc.bound(case[2], case[3], cd), case[0]
    for case in rc.general_cases():
        (_, cd, itd, sd), (_, ce, ite, se) = device_result(case), solve_one(case, emu)
        print(f"{case[0]}: device {cd!r} ({itd}) emulation {ce!r} ({ite})")
        assert sd == se == 0 and abs(itd - ite) <= 1 and abs(cd - ce) <= rc.bound(case[2], case[3], cd), case[0]


def test_paths_of_one_call_do_not_affect_each_other():
    check_mixed_call(rc.device_solver())


def test_wide_call():
    """300 workgroups, each with a workspace slab of its own, on 256 compute units"""
    check_wide_call(rc.device_solver())


@pytest.mark.parametrize("n", [3, 6])
def test_line_through_polytopes_by_region_keys(n):
    """end to end as the rounding step calls it: regions by key, the start points from the device's own centre LPs (of boxes of
    half-width 1e-6 cut by rows of norm 1e-2 .. 1e2), one restriction; the cost against the exact one within the bound"""
    case = next(c for c in rc.family("line") if c[0] == f"line-n{n}-k6-m{n + 2}")
    _, _, polys, path, exact = case
    keys = ['s', 't'] + [f"r{i}" for i in range(len(polys) - 2)]
    As = {v: polys[i][0] for i, v in enumerate(keys)}
    bs = {v: polys[i][1] for i, v in enumerate(keys)}
    by_key = [keys[i] for i in path]
    (cost, xs), = R.solve_path_restrictions_device(As, bs, n, [by_key])
    print(f"{case[0]}: cost {cost!r} exact {exact!r} bound {rc.bound(polys, path, cost):.3e}")
    assert xs is not None and set(xs) == set(by_key)
    pts = np.array([xs[by_key[0]][:n]] + [xs[v][n:] for v in by_key])
    rc.assert_points_feasible(polys, path, pts)
    assert all(np.array_equal(xs[by_key[j]][n:], xs[by_key[j + 1]][:n]) for j in range(len(by_key) - 1))
    assert abs(cost - exact) <= rc.bound(polys, path, cost), cost - exact


def test_iteration_limit_is_a_failure():
    case = rc.staircase(3)
    _, n, polys, path, _ = case
    pts, cost, its, st = rc.device_solver()(n, polys, [path], [rc.host_start(polys, path)], max_iter=3)
    assert st[0] == -1 and its[0] == 3 and np.isinf(cost[0]) and np.all(np.isfinite(pts[0]))


def test_bad_arguments():
    from gcs_admm_amd.scene import DeviceScene, GcsAdmmError
    n, polys, paths, starts = mixed_call()
    with DeviceScene(polys) as sc:
        for bad in (len(polys), -1):
            with pytest.raises(GcsAdmmError, match=r"out of range \(status 1\)"):
                sc.restrict_paths([[0, bad, 1]], [np.zeros((4, n))])
        with pytest.raises(GcsAdmmError, match=r"at least one region \(status 1\)"):
            sc.restrict_paths([[], [0, 1]], [np.zeros((1, n)), np.zeros((3, n))])
        pts, cost, its, st = sc.restrict_paths([], [])                       # no paths: nothing to do
        assert len(pts) == 0 and len(cost) == 0
        pts, cost, its, st = sc.restrict_paths(paths[:2], starts[:2])        # the scene still serves after a refusal
        assert list(st) == [0, 0]


def rounding_inputs(activations, name):
    As, bs, n, _, _ = fixture_sets(name)
    V, E, y_e = activations[name]
    return y_e, V, E, {v: [e for e in E if e[0] == v] for v in V}, As, bs, n


@pytest.mark.parametrize("name", BENCHMARKS)
def test_rounding_on_the_device(activations, name):
    y_e, V, E, I_out, As, bs, n = rounding_inputs(activations, name)
    cost, xv, yv = R.rounding(y_e, V, E, I_out, As, bs, n, restriction="device")
    cost_h, _, _ = R.rounding(y_e, V, E, I_out, As, bs, n)
    print(f"{name}: device {cost!r} host {cost_h!r} record {rc.RECORDS[name]}")
    assert abs(cost - rc.RECORDS[name]) <= 1e-5 * rc.RECORDS[name]
    on_path = [v for v in V if yv[v]]
    assert abs(cost - cost_h) <= 2.0 * (path_bound(As, on_path) + 1e-12 * max(1.0, cost))
    assert yv['s'] == 1 and yv['t'] == 1
    for v in on_path:
        for half in (xv[v][:n], xv[v][n:]):
            assert np.all(As[v] @ half <= bs[v] + 1e-9 * np.maximum(1.0, np.abs(bs[v])))


def test_rounding_many_equals_rounding_alone(activations):
    y_e, V, E, I_out, As, bs, n = rounding_inputs(activations, "benchmark4")
    problems = [dict(y_e_sol=y_e, V=V, E=E, I_v_out=I_out, As=As, bs=bs, n=n, seed=seed) for seed in range(8)]
    many = R.rounding_many(problems)
    for seed, (cost, xv, yv) in enumerate(many):
        c1, x1, y1 = R.rounding(y_e, V, E, I_out, As, bs, n, seed=seed, restriction="device")
        assert cost == c1 and yv == y1 and all(np.array_equal(xv[v], x1[v]) for v in V), seed
        assert abs(cost - rc.RECORDS["benchmark4"]) <= 1e-5 * rc.RECORDS["benchmark4"]


def test_cli_rounds_on_the_device(tmp_path):
    sys.path.insert(0, os.path.join(rc.ROOT, "tools"))
    from pkl_reader import load_data
    name = "benchmark1"
    r = subprocess.run([sys.executable, os.path.join(rc.ROOT, "admm_solver_v3.py"), "--test_file", name, "--show_plot", "False", "--rounding", "device"],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    rec = load_data(str(tmp_path / "benchmark_data" / f"admm_solver_v3_{name}.pkl"))
    n = 2
    length = sum(float(np.linalg.norm(np.asarray(rec["x_v_rounded"][v])[:n] - np.asarray(rec["x_v_rounded"][v])[n:]))
                 for v in rec["x_v_rounded"] if rec["y_v_rounded"][v] == 1)
    gold = load_fixture(name)[0]["golden_v3"]
    gx, gy = np.array(gold["x_v_rounded"]), np.array(gold["y_v_rounded"])
    glen = sum(np.linalg.norm(gx[i][:n] - gx[i][n:]) for i in range(len(gy)) if gy[i] == 1)
    assert abs(length - glen) <= 1e-5 * glen
