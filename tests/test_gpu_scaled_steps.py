"""The vertex-step kernels against the oracle, solve by solve, under the penalty schedule of tests/scaled_cases.py (rho 1, 3, 9, 4.5,
2.25; dual scale 1 / 3 or 3 on the step of each change) and with f32 state under the "nearest" rule of tests/solve_agreement.py.

Every step copies the oracle's state to the handle (f32: the f32-rounded state, which the oracle then solves from too), runs the
vertex step on the device and the oracle's, and lets the handle's own control step -- the one that moves the Newton counters into
the control block, solve_agreement.device_newton -- produce the (rho, mu_scale) of the next step from sums that force its increase
or decrease branch; the result is asserted bit for bit against the schedule.  Each run is judged three ways
(scaled_cases.Judgement): per-solve agreement, the run's warm Newton total, and the steps after a change of rho as cold steps
(per-step totals within one: no record is comparable there).  The closed-form vertices' columns are held to 1e-12 (f32 state: an
excess of 1e-12 over the f32 nearest the oracle's word).

The thresholds are the host builds' (tests/test_scaled_steps.py runs the same programs on the CPU; solve_agreement.py states their
scores).  Every test prints its summary."""
import numpy as np
import pytest

from gcs_admm_amd import IPM_TOL
from scaled_cases import TAU_DECR, TAU_INCR, Judgement, graph, pattern
from solve_agreement import device_newton, f32_round, generic_mask, nearest_excess, oracle_step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _expect(q, ws, expect):
    """what the handle must have planned for the case to test what its name says"""
    if expect == "wavefront":
        assert q["num_waves"] > 0 and q["num_workgroup_vertices"] == 0, q
    elif expect == "workgroup":
        assert q["num_workgroup_vertices"] > 0 and q["num_waves"] == 0, q
    elif expect == "split":
        assert q["num_workgroup_vertices"] == 0 and ws["num_split_vertices"] > 0, (q, ws)
    elif expect == "workgroup vertices":
        assert q["num_workgroup_vertices"] >= 1, q


def run(torch, oracle_lib, name, steps, dtype="f64", expect=None, region=False, **kw):
    from gcs_admm_amd.solver import DeviceSolver
    g = graph(name)
    f32 = dtype == "f32"
    d = DeviceSolver(g, dtype, device=0, **kw)
    _expect(d.query(), d.query_workspace(), expect)
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL)
    d.reset(tau_incr=TAU_INCR, tau_decr=TAU_DECR)
    solves = generic_mask(g)
    if region:
        solves[[g.src, g.dst]] = True              # region terminals: their kernel's solves are judged with the others
    closed = np.zeros(2 * g.num_edges, bool)       # the columns of the closed-form vertices
    for v in np.nonzero(~solves)[0]:
        closed[g.inc_ptr[v]:g.inc_ptr[v + 1]] = True
    perm = torch.from_numpy(d.col_of).to(d.device)          # incidence column -> state column (edge-major handles)
    label = f"{name} {dtype} {kw} {'schedule' if len(steps) > 12 else 'rho = 1'}"
    j = Judgement(label, f32="nearest" if f32 else False)
    for rho, mu_scale, change in steps:
        if f32:           # both sides solve from the state the device stores
            o.zedge[...] = f32_round(o.zedge); o.mu[...] = f32_round(o.mu)
        d.zedge.copy_(torch.from_numpy(o.zedge)); d.mu[:, perm] = torch.from_numpy(o.mu).to(d.mu.dtype).to(d.device)
        cb = d.read_control()
        assert cb.rho == rho and cb.mu_scale == mu_scale, (cb.rho, cb.mu_scale, rho, mu_scale)
        d.vertex_step()
        fails_ref, total_ref, _ = oracle_step(o, rho, mu_scale)
        got = d.copy[:, perm].double().cpu().numpy()
        assert np.isfinite(got).all()
        if closed.any():
            off = nearest_excess(got[:, closed], o.copy[:, closed]) if f32 else np.abs(got[:, closed] - o.copy[:, closed])
            assert off.max() <= 1e-12, (label, rho, mu_scale, off.max())
        total, fails = device_newton(d, rho, change, TAU_INCR, TAU_DECR)
        j.add(g, solves, rho, got, d.yv.cpu().numpy(), o.copy, o.yv, total, total_ref, fails, fails_ref)
        o.edge_step(mu_scale)
    d.close()
    print(j.summary())
    j.check()


F64_CASES = [
    ("benchmark4", "wavefront", dict(program="wavefront")),
    ("benchmark4", "workgroup", dict(program="workgroup")),
    ("benchmark4", "split", dict(program="workgroup", vertex_workspace=2)),
    ("benchmark1", None, dict(program="auto")),
    ("lattice 5x4", "wavefront", dict(program="wavefront")),       # (canonical boxes: the wavefront program's box variant)
    ("lattice n=3", "workgroup", dict(program="workgroup")),       # (n = 3, 6 lattices of canonical boxes: the BOX instantiation)
    ("lattice n=6", "workgroup", dict(program="workgroup")),
    ("star 40", "workgroup vertices", dict(program="auto")),
]


@pytest.mark.parametrize("name,expect,kw", F64_CASES, ids=[f"{n}-{e}" for n, e, _ in F64_CASES])
def test_vertex_steps_under_the_schedule(torch_gpu, oracle_lib, name, expect, kw):
    run(torch_gpu, oracle_lib, name, pattern("schedule"), expect=expect, **kw)


def test_region_terminals_under_the_schedule(torch_gpu, oracle_lib):
    """the terminal kernel has its own test of the record's rho (terminal_region.h): one scene whose terminals are regions, their
    solves in the mask"""
    run(torch_gpu, oracle_lib, "region scene", pattern("schedule"), region=True)


F32_CASES = [
    ("benchmark4", "wavefront", dict(program="wavefront", columns="incidence")),
    ("benchmark4", "wavefront", dict(program="wavefront", columns="edge")),
    ("lattice 14x11", "wavefront", dict(program="wavefront")),
    ("benchmark3", "workgroup", dict(program="workgroup")),
    ("lattice n=3", "workgroup", dict(program="workgroup")),
    ("lattice n=6", "workgroup", dict(program="workgroup")),
    ("intervals", None, dict()),
    ("benchmark4", "split", dict(program="workgroup", vertex_workspace=2)),
    ("star 40", "workgroup vertices", dict(program="auto")),
]


@pytest.mark.parametrize("steps", ["rho = 1", "schedule"])
@pytest.mark.parametrize("name,expect,kw", F32_CASES, ids=[f"{n}-{e}-{k.get('columns', '')}" for n, e, k in F32_CASES])
def test_vertex_steps_with_f32_state(torch_gpu, oracle_lib, name, expect, kw, steps):
    run(torch_gpu, oracle_lib, name, pattern(steps), dtype="f32", expect=expect, **kw)
