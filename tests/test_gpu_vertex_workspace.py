"""Vertex sub-problems larger than LDS (gcsadmm_graph_desc.vertex_workspace): the split form of the workgroup program, whose edge
blocks live in a device-memory workspace (csrc/vertex_wg.h wg_solve_vertex<..., SPLIT>).  Checked on an MI355X:
  * mode 2 (every workgroup-program vertex split) against mode 0 on graphs that fit: the same arithmetic, so the same bits;
  * mode 1 on the bench workloads: nothing fits worse than before, so nothing moves;
  * oversized hubs, which mode 0 refuses, against the CPU oracle step by step and over whole runs, warm and cold;
  * a graph on which the wavefront, workgroup and split launches all run, through run, run_timed and the partitioned loop."""
import numpy as np
import pytest

from gcs_admm_amd import IPM_TOL
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import graph_from_sets, lattice_boxes, sets_of_graph
from solve_agreement import Agreement, NewtonParity, device_newton, generic_mask, oracle_step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _solver(g, dtype="f64", **kw):
    from gcs_admm_amd.solver import DeviceSolver
    return DeviceSolver(g, dtype, device=0, **kw)


def hub_case(n, spokes, generic=False, facets=None, seed=0):
    """a hub polytope in R^n overlapping `spokes` small boxes on a ring, an edge each way to every spoke (hub degree 2 spokes); s and t
    are points in two spokes.  generic: the hub is a rotated box (2n facets, no canonical box: the generic instantiation); `facets`
    > 2n adds random tangent cuts at distance 1.5 (they keep the hub's inscribed ball)."""
    from gcs_admm_amd.graph import convert_pt_to_polytope
    rng = np.random.default_rng(seed)
    E = np.vstack([np.eye(n), -np.eye(n)])
    if generic:
        R, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A = np.vstack([R, -R])
        if facets and facets > 2 * n:
            extra = rng.standard_normal((facets - 2 * n, n))
            A = np.vstack([A, extra / np.linalg.norm(extra, axis=1, keepdims=True)])
        b = np.hstack([np.ones(2 * n), np.full(A.shape[0] - 2 * n, 1.5)])
    else:
        A, b = E, np.ones(2 * n)
    As, bs, edges = {0: A}, {0: b}, []
    for k in range(spokes):
        c = np.zeros(n); ang = 2 * np.pi * k / spokes
        c[0], c[1] = 1.1 * np.cos(ang), 1.1 * np.sin(ang)
        c[2:] = rng.uniform(-0.2, 0.2, n - 2)
        h = rng.uniform(0.3, 0.4, n)
        As[k + 1], bs[k + 1] = E, np.hstack([c + h, -c + h])
        edges += [(0, k + 1), (k + 1, 0)]
    cs = 0.5 * (bs[1][:n] - bs[1][n:]); ct = 0.5 * (bs[spokes][:n] - bs[spokes][n:])
    As['s'], bs['s'] = convert_pt_to_polytope(cs)
    As['t'], bs['t'] = convert_pt_to_polytope(ct)
    edges += [('s', 1), (spokes, 't')]
    keys = ['s', 't'] + list(range(spokes + 1))
    return graph_from_sets({k: As[k] for k in keys}, {k: bs[k] for k in keys}, n, edges=edges)


def star(k):
    from conftest import star_case
    As, bs, n = star_case(k)
    return graph_from_sets(As, bs, n)


def mixed_case():
    """a 60 x 50 box lattice (3 000 cells: the wavefront program) with two hubs on top: one over ~80 cells (degree > 150: the split
    form) and one over ~40 (degree > 63, fits LDS: the workgroup program)"""
    g0 = lattice_boxes(60, 50, seed=3)
    As, bs = sets_of_graph(g0)
    As, bs = {k: np.array(v) for k, v in As.items()}, {k: np.array(v) for k, v in bs.items()}
    edges = list(g0.edges_as_keys())
    A = np.vstack([np.eye(2), -np.eye(2)])
    for name, (x0, x1, y0, y1) in (("hub", (20.2, 29.8, 10.2, 17.8)), ("hub2", (40.2, 45.8, 30.2, 36.8))):
        As[name], bs[name] = A, np.array([x1, y1, -x0, -y0])
        for k in g0.keys:
            if k in ('s', 't'):
                continue
            b = bs[k]
            if b[0] > x0 and -b[2] < x1 and b[1] > y0 and -b[3] < y1:
                edges += [(name, k), (k, name)]
    return graph_from_sets(As, bs, 2, edges=edges)


def _state(d):
    return [t.cpu().numpy().copy() for t in (d.copy, d.mu, d.zedge, d.xv, d.zv, d.yv)]


def _steps_equal(ga, gb, steps):
    """k vertex + edge steps on both handles from the same zero state: the same state arrays and control counters after them"""
    for d in (ga, gb):
        d.reset(max_it=100)
    for _ in range(steps):
        for d in (ga, gb):
            d.vertex_step(); d.edge_step(); d.control()
    sa, sb = _state(ga), _state(gb)
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    ca, cb = ga.read_control(), gb.read_control()
    assert ca.inner_iters == cb.inner_iters and ca.inner_failures == cb.inner_failures == 0


BITWISE = [
    ("benchmark4", lambda: load_fixture("benchmark4")[1], "f64", {}),
    ("lattice n=3 box", lambda: lattice_boxes(8, 6, n=3, seed=1), "f64", {}),
    ("lattice n=6 box", lambda: lattice_boxes(6, 5, n=6, seed=1), "f64", {}),
    ("lattice n=6 generic", lambda: lattice_boxes(6, 5, n=6, seed=1), "f64", dict(wave_generic_rows=1)),
    ("lattice n=8", lambda: lattice_boxes(5, 4, n=8, seed=1), "f64", {}),
    ("lattice n=3 f32", lambda: lattice_boxes(8, 6, n=3, seed=2), "f32", {}),
]


@pytest.mark.parametrize("name,make,dtype,kw", BITWISE, ids=[c[0] for c in BITWISE])
def test_split_form_is_bitwise_the_in_lds_form(torch_gpu, name, make, dtype, kw):
    """mode 2 puts every workgroup-program vertex in the split form (256 threads); against mode 0 on the 256-thread build
    (workgroup256) the arithmetic is the same in the same order: the same bits after 5 steps and over a whole run"""
    g = make()
    a = _solver(g, dtype, program="workgroup256", **kw)
    b = _solver(g, dtype, program="workgroup256", vertex_workspace=2, **kw)
    qa, qb = a.query(), b.query()
    wb = b.query_workspace()
    assert qb["num_workgroup_vertices"] == 0 and wb["num_split_vertices"] == qa["num_workgroup_vertices"] > 0
    assert wb["workspace_bytes"] > 0 and wb["split_lds_bytes"] < qa["workgroup_lds_bytes"]
    _steps_equal(a, b, 5)
    ra, rb = a.solve(max_it=300), b.solve(max_it=300)
    assert ra["iterations"] == rb["iterations"]
    assert np.array_equal(a.trace.cpu().numpy(), b.trace.cpu().numpy())
    # (against mode 0 at its automatic thread count -- 512 on these small graphs, another reduction tree -- the in-LDS program itself
    #  differs from its 256-thread build by round-off: ~5e-12 of the arrays' magnitude after 5 steps at n = 6, 8)


@pytest.mark.parametrize("workload", ["benchmark4", "s10k", "s6d", "s100k"])
def test_mode_1_changes_nothing_that_fits(torch_gpu, workload):
    import bench
    g, dtype, _ = bench.make_workload(workload)
    columns = "edge" if g.num_edges >= 20000 else "incidence"
    a = _solver(g, dtype, columns=columns)
    b = _solver(g, dtype, columns=columns, vertex_workspace=1)
    assert a.query() == b.query()
    assert b.query_workspace() == dict(num_split_vertices=0, split_lds_bytes=0, workspace_bytes=0)
    _steps_equal(a, b, 1)


HUBS = [
    ("n=2 degree 120", lambda: star(60)),
    ("n=2 degree 200", lambda: star(100)),
    ("n=6 generic degree 30, 12 facets", lambda: hub_case(6, 15, generic=True)),
    ("n=7 degree 18", lambda: hub_case(7, 9)),      # (degree 16 still fits LDS at n = 7)
    ("n=8 degree 16", lambda: hub_case(8, 8)),
]


@pytest.mark.parametrize("cold", [False, True], ids=["warm", "cold"])
@pytest.mark.parametrize("name,make", HUBS, ids=[c[0] for c in HUBS])
def test_oversized_hub_against_oracle(torch_gpu, oracle_lib, name, make, cold):
    from gcs_admm_amd.solver import GcsAdmmError
    g = make()
    with pytest.raises(GcsAdmmError, match="does not fit the 160 KB"):
        _solver(g)
    d = _solver(g, vertex_workspace=1)
    assert d.query_workspace()["num_split_vertices"] == 1
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL, warm_start=not cold)
    d.reset(cold_start=cold)
    torch = torch_gpu
    diffs = []
    gen = generic_mask(g)
    mode = "cold" if cold else "warm"
    agree, newton = Agreement(f"{name} {mode}"), NewtonParity(f"{name} {mode}")
    for it in range(24):        # (a hub and its spokes: few generic vertices, so more steps for the per-solve statistic)
        d.zedge.copy_(torch.from_numpy(o.zedge)); d.mu.copy_(torch.from_numpy(o.mu))
        d.vertex_step()
        fails, iters, _ = oracle_step(o)
        assert fails == 0
        copy = d.copy.cpu().numpy()
        assert np.isfinite(copy).all()
        diffs.append(np.abs(copy - o.copy).max())
        assert np.abs(d.yv.cpu().numpy() - o.yv).max() <= 5e-4
        agree.add(g, gen, copy, d.yv.cpu().numpy(), o.copy, o.yv)
        it_dev, fails_dev = device_newton(d)
        newton.add(it_dev, iters, fails_dev, fails)
        d.copy.copy_(torch.from_numpy(o.copy))
        d.edge_step(); o.edge_step(1.0)
    diffs = np.array(diffs)
    assert diffs.max() <= 2e-3 and np.median(diffs) <= 1e-5, (diffs.max(), np.median(diffs))
    agree.check()
    newton.check(cold)
    res = d.solve(max_it=400, cold_start=cold)
    ora = oracle_lib.Oracle(g, ipm_tol=IPM_TOL, warm_start=not cold).run(max_it=400)
    assert res["inner_failures"] == 0 and res["iterations"] == ora["iterations"]
    # (n = 2 degree 120, cold: one iteration of the run (189 of 230) lies outside the bound on both residuals, 19 % on the dual one;
    #  every other entry is inside it, and the same trace comes out whether the other vertices run in LDS at 512 threads, split at 256
    #  threads or on the wavefront program -- the sensitivity of that run, not of the split form.  Pinned as it stands.)
    loose = 2 if (name, cold) == ("n=2 degree 120", True) else 0
    for key in ("pri_res_seq", "dual_res_seq"):
        out = np.abs(res[key] - ora[key]) > 2e-4 + 1e-3 * np.abs(ora[key])
        assert out.sum() <= loose, (key, np.nonzero(out)[0])
        assert np.all(np.abs(res[key] - ora[key]) <= 2e-4 + 0.2 * np.abs(ora[key])), key


def test_mixed_graph_all_three_launches(torch_gpu, oracle_lib):
    """wavefront program (the lattice), workgroup program in LDS (the degree-80 hub) and split form (the degree-160 hub) in one
    vertex step, through gcsadmm_run, gcsadmm_run_timed and the single-rank gcsadmm_run_partitioned, against the oracle"""
    g = mixed_case()
    deg = np.diff(g.inc_ptr)
    assert sorted(deg)[-2:][0] > 63 and deg.max() > 150
    d = _solver(g, vertex_workspace=1)
    q, w = d.query(), d.query_workspace()
    assert q["num_waves"] > 0 and q["num_workgroup_vertices"] == 1 and w["num_split_vertices"] == 1
    # the three launches of one vertex step, step by step along an oracle run: the per-solve contract and the warm Newton total
    torch = torch_gpu
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL)
    d.reset()
    gen = generic_mask(g)
    agree, newton = Agreement("mixed"), NewtonParity("mixed warm")
    for it in range(10):
        d.zedge.copy_(torch.from_numpy(o.zedge)); d.mu.copy_(torch.from_numpy(o.mu))
        d.vertex_step()
        fails, iters, _ = oracle_step(o)
        agree.add(g, gen, d.copy.cpu().numpy(), d.yv.cpu().numpy(), o.copy, o.yv)
        it_dev, fails_dev = device_newton(d)
        newton.add(it_dev, iters, fails_dev, fails)
        o.edge_step(1.0)
    agree.check()
    newton.check_warm()
    kw = dict(max_it=60, eps_abs=0.0, eps_rel=0.0)
    ora = oracle_lib.Oracle(g, ipm_tol=IPM_TOL).run(**kw)
    ref = None
    for timed in (False, True):
        res = d.solve(timed=timed, **kw)
        assert res["inner_failures"] == 0
        for key in ("pri_res_seq", "dual_res_seq"):
            assert np.all(np.abs(res[key] - ora[key]) <= 2e-4 + 1e-3 * np.abs(ora[key])), key
        tr = d.trace.cpu().numpy()
        if ref is None:
            ref = tr
        else:
            assert np.array_equal(tr, ref)      # timing the launches changes nothing
    p = _solver(g, vertex_workspace=1)
    p.attach_comm(0, 1, p.unique_id(), {}, {})
    cb = p.solve_partitioned(**kw)
    assert cb.it == 61 and cb.inner_failures == 0
    assert np.array_equal(p.trace.cpu().numpy(), ref)
