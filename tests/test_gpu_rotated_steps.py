"""The workgroup vertex kernels on ROTATED polytopes in R^3 .. R^8 (tests/rotated_cases.py): the dense-row path of the generic
instantiation, which the lattices of canonical boxes leave untested outside n = 2 (every off-diagonal facet product is an exact zero
there).  Each case is 14 vertices x 12 steps, copied from the oracle's state every step as in test_gpu_scaled_steps.py.

  * plan: the handle runs every generic vertex on the workgroup program, generic instantiation (a rotated box is no canonical box);
  * parity with the oracle on the same rotated graph, warm, rho = 1: scaled_cases.Judgement.check();
  * equivariance, cold: the oracle solves the AXIS-ALIGNED lattice, its state is rotated into the handle every step, and the handle's
    copy columns are held to the rotated columns of the oracle -- a reference that shares none of the dense-row arithmetic;
  * the seeds whose vertex 13 ended in a non-finite Newton step before gcs_math::step_finite: no inner failure through step 8;
  * the split form (units in the device-memory workspace) and f32 state under the "nearest" rule, one n = 6 case each.

Thresholds: solve_agreement.py, unchanged (tests/test_rotated_steps.py runs the host build of the same program on the same cases; its
docstring and solve_agreement.py state the scores).  Every test prints its summary."""
import numpy as np
import pytest

from gcs_admm_amd import IPM_TOL
from rotated_cases import CASES, STEPS, case_id, rotate_state, rotated_pair
from scaled_cases import Judgement
from solve_agreement import device_newton, f32_round, generic_mask, nearest_excess, oracle_step

pytestmark = pytest.mark.gpu

BY_N = {(c[0], c[3] > 0): c for c in CASES}       # (n, has cuts) -> case
FAILED_BEFORE = [c for c in CASES if c[0] >= 5 and c[3] == 0]


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _handle(g, dtype="f64", split=False, **kw):
    """a handle that runs every generic vertex of g on the workgroup program (split: from the device-memory workspace)"""
    from gcs_admm_amd.solver import DeviceSolver
    d = DeviceSolver(g, dtype, device=0, program="workgroup", vertex_workspace=2 if split else 0, **kw)
    q, ws = d.query(), d.query_workspace()
    n_generic = int(generic_mask(g).sum())
    assert q["num_waves"] == 0, q
    if split:
        assert q["num_workgroup_vertices"] == 0 and ws["num_split_vertices"] == n_generic, (q, ws)
    else:
        assert q["num_workgroup_vertices"] == n_generic == 12 and ws["num_split_vertices"] == 0, (q, ws)
    return d


def _closed_columns(g, solves):
    closed = np.zeros(2 * g.num_edges, bool)
    for v in np.nonzero(~solves)[0]:
        closed[g.inc_ptr[v]:g.inc_ptr[v + 1]] = True
    return closed


def run(torch, oracle_lib, case, steps=STEPS, dtype="f64", cold=False, equivariance=False, split=False):
    """the Judgement (scaled_cases.py; rho = 1 throughout) of `steps` vertex steps of a handle on the rotated graph of `case`.  equivariance: the oracle runs the
    axis-aligned graph and its state and columns are rotated; otherwise it runs the rotated graph itself."""
    g0, g, Q = rotated_pair(*case)
    to_rot = (lambda a: rotate_state(a, Q)) if equivariance else (lambda a: a)
    f32 = dtype == "f32"
    d = _handle(g, dtype, split)
    o = oracle_lib.Oracle(g0 if equivariance else g, ipm_tol=IPM_TOL, warm_start=not cold)
    d.reset(cold_start=cold)
    solves = generic_mask(g)
    closed = _closed_columns(g, solves)
    perm = torch.from_numpy(d.col_of).to(d.device)
    label = f"{case_id(case)} {dtype} {'cold' if cold else 'warm'}{' equivariance' if equivariance else ''}{' split' if split else ''}"
    j = Judgement(label, f32="nearest" if f32 else False)
    for _ in range(steps):
        if f32:           # both sides solve from the state the device stores
            o.zedge[...] = f32_round(o.zedge); o.mu[...] = f32_round(o.mu)
        d.zedge.copy_(torch.from_numpy(to_rot(o.zedge))); d.mu[:, perm] = torch.from_numpy(to_rot(o.mu)).to(d.mu.dtype).to(d.device)
        d.vertex_step()
        fails_ref, total_ref, _ = oracle_step(o)
        got = d.copy[:, perm].double().cpu().numpy()
        want = to_rot(o.copy)
        assert np.isfinite(got).all()
        if not equivariance:      # (the closed-form vertices: the point terminals' columns)
            off = nearest_excess(got[:, closed], want[:, closed]) if f32 else np.abs(got[:, closed] - want[:, closed])
            assert off.max() <= 1e-12, (label, off.max())
        total, fails = device_newton(d)
        j.add(g, solves, 1.0, got, d.yv.cpu().numpy(), want, o.yv, total, total_ref, fails, fails_ref)
        o.edge_step(1.0)
    d.close()
    print(j.summary())
    return j


@pytest.mark.parametrize("n", [3, 6])
def test_rotated_boxes_run_the_generic_instantiation(torch_gpu, n):
    """n = 3, 6 have a BOX instantiation: the lattice takes it (smaller LDS layout), the rotated lattice must not -- its layout is the one
    the lattice gets with the generic rows forced"""
    from gcs_admm_amd.solver import DeviceSolver
    case = BY_N[(n, False)]
    g0, g, _ = rotated_pair(*case)
    lds = {}
    for name, graph, kw in (("rotated", g, {}), ("lattice", g0, {}), ("lattice, generic rows", g0, dict(wave_generic_rows=1))):
        d = _handle(graph, **kw)
        lds[name] = d.query()["workgroup_lds_bytes"]
        d.close()
    print(lds)
    assert lds["rotated"] == lds["lattice, generic rows"] > lds["lattice"], lds


@pytest.mark.parametrize("case", [BY_N[(n, False)] for n in (3, 5, 6, 7, 8)] + [BY_N[(4, True)], BY_N[(8, True)]], ids=case_id)
def test_rotated_vertex_steps_against_the_oracle(torch_gpu, oracle_lib, case):
    run(torch_gpu, oracle_lib, case).check()


@pytest.mark.parametrize("case", [BY_N[(n, False)] for n in (3, 6, 8)], ids=case_id)
def test_rotated_vertex_steps_are_the_rotated_axis_aligned_solves(torch_gpu, oracle_lib, case):
    j = run(torch_gpu, oracle_lib, case, cold=True, equivariance=True)
    j.agree.check()
    j.newton.check_cold()


@pytest.mark.parametrize("cold", [True, False], ids=["cold", "warm"])
@pytest.mark.parametrize("case", FAILED_BEFORE, ids=case_id)
def test_seeds_that_ended_in_a_nonfinite_step(torch_gpu, oracle_lib, case, cold):
    """run to step 8 (the failures were at steps 5 - 8): no inner failure in the handle's counters, none in the oracle"""
    newton = run(torch_gpu, oracle_lib, case, steps=9, cold=cold).newton
    assert sum(newton.fails) == 0 and sum(newton.fails_ref) == 0, newton.summary()


def test_rotated_vertex_steps_from_the_workspace(torch_gpu, oracle_lib):
    run(torch_gpu, oracle_lib, BY_N[(6, False)], split=True).check()


def test_rotated_vertex_steps_with_f32_state(torch_gpu, oracle_lib):
    run(torch_gpu, oracle_lib, BY_N[(6, False)], dtype="f32").check()
