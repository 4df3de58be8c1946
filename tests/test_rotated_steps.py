"""Vertex solves on rotated polytopes in R^3 .. R^8 (tests/rotated_cases.py), on the CPU: the workgroup program's host build
(tests/hostemu/wg_emu.cpp, generic instantiation: dense facet rows) and the oracle.

(a) Against the oracle on the SAME rotated graph, from identical state, 12 steps, warm and cold, tasks ascending and descending: every
    solve by Agreement.check() and the Newton iterations by NewtonParity.check(cold), with the constants of solve_agreement.py; no
    inner failure on either side.
(b) Equivariance, cold: the oracle runs the AXIS-ALIGNED lattice (canonical boxes plus the unrotated cut rows: none of the dense-row
    code under test, none of its own off-diagonal terms either); every step its state is rotated into the rotated graph, the host build
    solves that cold, and the result is compared with the rotated copy columns of the oracle (both point blocks rotated, y as it is)
    by the same Agreement.check() and check_cold().  Warm equivariance is not judged: each side would restart from its own record,
    and the oracle against itself then scores 0.26 - 0.30 within 1e-9.
(c) Failure census: 8 (lattice, rotation) seed pairs x 30 steps, warm and cold, oracle and host build.  Before the rule of
    gcs_math::step_finite, runs with at least one inner failure, out of 16 per n:
        n = 5: oracle 2, host build 1     n = 6: 5, 4     n = 7: 8, 6     n = 8: 4, 5     n = 2, 3, 4 and every unrotated lattice: 0
    always vertex 13 (the cell that holds t, y_v -> 1), ADMM steps 5 - 8, after 10 - 12 Newton iterations of a cold solve (19 - 22
    with a failed warm attempt), status -3: the solve was finished but for the last digits (mu 3e-9 .. 1.2e-8 against 3e-9), one more
    Newton solve returned a non-finite direction, fmin / fmax in the ratio test dropped the NaNs, and a full step of NaNs was taken.
    E.g. (n, lattice, rotation) = (6, 2, 106) cold: step 5 failed at iteration 11 on both sides.  Now: zero everywhere.
    The wavefront program (n = 2 only) shows no failure on the rotated n = 2 cases and is unchanged; the workgroup program carries the
    rule in its dense-row instantiations for n >= 3 (rule 6).
(d) A seeded error that is the identity on boxes: ONE facet product of the K assembly of vertex_wg.h (facet 0, entry (1, 0)) times
    1 + 1e-3.  On the lattices of canonical boxes at n = 3, 6 the build is bit for bit the clean copy's (the product is an exact zero
    there) and meets the contract; on the rotated n = 3 and n = 6 cases judgements (a) and (b) both reject it (0.10 - 0.16 of the
    solves within 1e-9, 9 / 25 inner failures); the clean copy passes both.

Measured (host build, 12 steps; near / close / worst; per-vertex Newton counts equal) -- see solve_agreement.py for the table."""
import os

import numpy as np
import pytest

from gcs_admm_amd import IPM_TOL
from gcs_admm_amd.graph import lattice_boxes
from hostemu_lib import emu_library
from mutant_build import build_mutants
from rotated_cases import CASES, REPRO, STEPS, case_id, census_seeds, rotate_state, rotated_graph, rotated_pair
from solve_agreement import Agreement, NewtonParity, generic_mask, oracle_step
from test_hostemu_wg import WarmRecords, wg_step

HERE = os.path.dirname(os.path.abspath(__file__))
FWD, REV = ("wgemu", "wg_emu_vertex_step"), ("wgemu_rev", "wg_emu_vertex_step_rev")


@pytest.fixture(scope="module")
def pairs():
    """{case: (axis-aligned graph, rotated graph, Q)}, built once"""
    return {c: rotated_pair(*c) for c in CASES}


def run_same_graph(oracle_lib, lib, fn, g, cold, label, steps=STEPS):
    """(a): lib's vertex step and the oracle's on g from the oracle's state"""
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL, warm_start=not cold)
    w = None if cold else WarmRecords(emu_library(FWD[0]), g)      # (the record's size: the same in every build)
    agree, newton = Agreement(label), NewtonParity(label)
    for _ in range(steps):
        a = wg_step(lib, fn, g, o.zedge.copy(), o.mu.copy(), warm=w)
        fails, iters, per_vertex = oracle_step(o)
        gen = a[5]
        assert np.array_equal(gen, generic_mask(g))
        agree.add(g, gen, a[0], a[3], o.copy, o.yv)
        newton.add(a[4][1], iters, a[4][0], fails, a[7][gen], per_vertex[gen])
        o.edge_step(1.0)
    return agree, newton


def run_equivariance(oracle_lib, lib, fn, pair, label, steps=STEPS):
    """(b): the oracle on the axis-aligned graph, lib cold on the rotated graph from the rotated state"""
    g0, g, Q = pair
    assert np.array_equal(g0.inc_ptr, g.inc_ptr) and np.array_equal(g0.inc_edge, g.inc_edge)
    o = oracle_lib.Oracle(g0, ipm_tol=IPM_TOL, warm_start=False)
    agree, newton = Agreement(label), NewtonParity(label)
    for _ in range(steps):
        a = wg_step(lib, fn, g, rotate_state(o.zedge, Q), rotate_state(o.mu, Q))
        fails, iters, per_vertex = oracle_step(o)
        gen = a[5]
        agree.add(g, gen, a[0], a[3], rotate_state(o.copy, Q), o.yv)
        newton.add(a[4][1], iters, a[4][0], fails, a[7][gen], per_vertex[gen])
        o.edge_step(1.0)
    return agree, newton


@pytest.mark.parametrize("cold", [False, True], ids=["warm", "cold"])
@pytest.mark.parametrize("order", [FWD, REV], ids=["ascending", "descending"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rotated_solves_meet_the_contract_against_the_oracle(oracle_lib, pairs, case, order, cold):
    g = pairs[case][1]
    assert sorted(set(np.diff(g.poly_ptr).tolist())) == sorted({2 * case[0], 2 * case[0] + case[3]})
    label = f"rotated {case_id(case)} {order[0]} {'cold' if cold else 'warm'}"
    agree, newton = run_same_graph(oracle_lib, emu_library(order[0]), order[1], g, cold, label)
    agree.check()
    newton.check(cold)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rotated_solves_are_the_rotated_axis_aligned_solves(oracle_lib, pairs, case):
    agree, newton = run_equivariance(oracle_lib, emu_library(FWD[0]), FWD[1], pairs[case], f"equivariance {case_id(case)} cold")
    agree.check()
    newton.check_cold()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rotated_cases_plan_the_generic_workgroup_instantiation(pairs, case):
    """what gcsadmm_create decides for the handle of test_gpu_rotated_steps.py: every generic vertex on the workgroup program, and the
    BOX instantiation (n = 3, 6) off -- a rotated box does not pass canonical_box; the axis-aligned lattice without cuts does"""
    import test_create_plan as P
    lib = P.load(P.build_lib())
    g0, g, _ = pairs[case]
    p = P.plan(lib, g, vertex_program=2)
    assert sorted(p.wg_vtx) == list(np.nonzero(generic_mask(g))[0]) and p.n_waves == 0 and p.wg_box == 0
    assert P.plan(lib, g0, vertex_program=2).wg_box == int(case[0] in (3, 6) and case[3] == 0)


def _census(oracle_lib, graphs, steps=30):
    """inner failures of the oracle and of the workgroup host build over `graphs`, warm and cold: two lists of (graph, mode, step, vertex)"""
    lib = emu_library(FWD[0])
    bad_oracle, bad_build = [], []
    for gi, g in enumerate(graphs):
        for cold in (True, False):
            o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL, warm_start=not cold)
            w = None if cold else WarmRecords(lib, g)
            for it in range(steps):
                a = wg_step(lib, FWD[1], g, o.zedge.copy(), o.mu.copy(), warm=w)
                fails, _, per_vertex = oracle_step(o)
                bad_build += [(gi, cold, it, int(v)) for v in np.nonzero(a[6])[0]]
                assert fails == (per_vertex < 0).sum() and a[4][0] == (a[6] != 0).sum()
                bad_oracle += [(gi, cold, it, int(v)) for v in np.nonzero(per_vertex < 0)[0]]
                o.edge_step(1.0)
    return bad_oracle, bad_build


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_census_of_rotated_lattices_has_no_inner_failure(oracle_lib, n):
    bad_oracle, bad_build = _census(oracle_lib, [rotated_graph(n, ls, rs) for ls, rs in census_seeds(n)])
    print(f"[census rotated n={n}] oracle failures {len(bad_oracle)} host build failures {len(bad_build)} over 8 seeds x 30 steps x 2")
    assert not bad_oracle and not bad_build, (bad_oracle[:4], bad_build[:4])


@pytest.mark.parametrize("n", [2, 5, 6, 7, 8])
def test_census_of_axis_aligned_lattices_has_no_inner_failure(oracle_lib, n):
    bad_oracle, bad_build = _census(oracle_lib, [lattice_boxes(4, 3, n=n, seed=ls) for ls, _ in census_seeds(n)])
    assert not bad_oracle and not bad_build, (bad_oracle[:4], bad_build[:4])


def test_census_of_the_wavefront_program_on_rotated_polygons(oracle_lib):
    """the wavefront program (vertex_program.inc, n = 2 only) has no rule for a non-finite step: on the rotated n = 2 cases none occurs"""
    from test_hostemu import WarmRecords as WaveRecords, emu_step
    lib = emu_library("emu")
    failures = 0
    for ls, rs in census_seeds(2):
        g = rotated_graph(2, ls, rs)
        for cold in (True, False):
            o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL, warm_start=not cold)
            w = None if cold else WaveRecords(g)
            for _ in range(30):
                failures += int(emu_step(lib, g, o.zedge.copy(), o.mu.copy(), 1.0, 1.0, warm=w)[4][0])
                failures += o.vertex_step(1.0, 1.0)
                o.edge_step(1.0)
    assert failures == 0


def test_the_repro_fails_no_solve_through_step_8(oracle_lib, pairs):
    """(6, lattice 2, rotation 106), cold: step 5 ended in a non-finite Newton step at iteration 11, status -3 (oracle: -111)"""
    g = pairs[REPRO][1]
    for cold in (True, False):
        _, newton = run_same_graph(oracle_lib, emu_library(FWD[0]), FWD[1], g, cold, f"repro {'cold' if cold else 'warm'}", steps=9)
        print(newton.summary())
        assert sum(newton.fails) == 0 and sum(newton.fails_ref) == 0


# ---- (d) a seeded error that is the identity on boxes
KSUM = "                    sk += (Da[i * m + j] + Db[i * m + j]) * aa;\n"
MUTANTS = {
    "clean": [],
    "offdiag": [(KSUM, KSUM.replace("* aa;", "* (j == 0 && k == 1 && l == 0 ? aa * (1.0 + 1e-3) : aa);"))],
}
MUTANT_CASES = [c for c in CASES if c[0] in (3, 6) and c[3] == 0]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    return build_mutants(tmp_path_factory.mktemp("rotated_mutants"), "vertex_wg.h", MUTANTS, os.path.join(HERE, "hostemu", "wg_emu.cpp"))


@pytest.mark.parametrize("n", [3, 6])
def test_seeded_offdiagonal_error_is_the_identity_on_boxes(oracle_lib, builds, n):
    """the lattice cases the suite had (test_hostemu_wg.py: lattice_boxes(4, 3, n, seed 1)): bit for bit the clean copy, contract met"""
    g = lattice_boxes(4, 3, n=n, seed=1)
    for cold in (False, True):
        o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL, warm_start=not cold)
        wa, wb = (None, None) if cold else (WarmRecords(builds["clean"], g), WarmRecords(builds["clean"], g))
        agree, newton = Agreement(f"offdiag on lattice n={n}"), NewtonParity(f"offdiag on lattice n={n}")
        for _ in range(6):
            a = wg_step(builds["clean"], FWD[1], g, o.zedge.copy(), o.mu.copy(), warm=wa)
            b = wg_step(builds["offdiag"], FWD[1], g, o.zedge.copy(), o.mu.copy(), warm=wb)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            fails, iters, per_vertex = oracle_step(o)
            agree.add(g, b[5], b[0], b[3], o.copy, o.yv)
            newton.add(b[4][1], iters, b[4][0], fails, b[7][b[5]], per_vertex[b[5]])
            o.edge_step(1.0)
        assert agree.legacy_ok()
        agree.check()
        newton.check(cold)


def _rejected(agree, newton, cold):
    try:
        newton.check(cold)
    except AssertionError:
        return True
    return bool(agree.failures())


@pytest.mark.parametrize("case", MUTANT_CASES, ids=case_id)
def test_rotated_cases_reject_the_seeded_offdiagonal_error(oracle_lib, builds, pairs, case):
    for name, want in (("clean", False), ("offdiag", True)):
        for cold in (False, True):
            agree, newton = run_same_graph(oracle_lib, builds[name], FWD[1], pairs[case][1], cold, f"{name} (a) {case_id(case)} cold={cold}")
            print(agree.summary()); print(newton.summary())
            assert _rejected(agree, newton, cold) == want, f"judgement (a), {name}, cold={cold}\n" + agree.summary()
        agree, newton = run_equivariance(oracle_lib, builds[name], FWD[1], pairs[case], f"{name} (b) {case_id(case)}")
        print(agree.summary()); print(newton.summary())
        assert _rejected(agree, newton, True) == want, f"judgement (b), {name}\n" + agree.summary()
