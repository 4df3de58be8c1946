"""The per-solve agreement contract (tests/solve_agreement.py) rejects subtle errors that the legacy statistic lets through.

The workgroup program's host build (tests/hostemu/wg_emu.cpp) is compiled from a copy of csrc/ whose gcs_math.h carries one seeded
error each -- the interior-point numerics every device solver shares -- and run for 12 steps from the oracle's state on benchmark4 and
benchmark1:
  * REG_DELTA x 1.1 (the Tikhonov term): legacy statistic passes (worst ~1e-4, median ~6e-6), 0.06 / 0.13 of solves within 1e-9;
  * Mehrotra centring r^3 -> r^3 (1 - 1e-3 r): legacy statistic passes (worst ~3e-5, median ~2e-6), 0.39 / 0.25 within 1e-9;
  * NT scaling eta x 1.01: a wrong but convergent Newton direction, seen in the iteration counts (totals +2.4 % / +7.4 % warm,
    +1.2 % / +2.0 % cold, per-vertex counts equal in 0.44 - 0.85 of the solves).
The clean copy passes the contract.  The four builds compile in parallel (~45 s of CPU time in all)."""
import os

import pytest

from gcs_admm_amd import IPM_TOL
from gcs_admm_amd.cases import load_fixture
from mutant_build import build_mutants
from solve_agreement import Agreement, NewtonParity, oracle_step
from test_hostemu_wg import WarmRecords, wg_step

HERE = os.path.dirname(os.path.abspath(__file__))

# (anchor in gcs_math.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "reg_delta": [("constexpr double REG_DELTA = 1e-7;", "constexpr double REG_DELTA = 1.1e-7;")],
    "centring": [("    return ratio * ratio * ratio;\n", "    return ratio * ratio * ratio * (1.0 - 1e-3 * ratio);\n")],
    "eta": [("eta = sqrt_nr((ss * is) * iz);", "eta = 1.01 * sqrt_nr((ss * is) * iz);")],
}
STEPS = 12


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    return build_mutants(tmp_path_factory.mktemp("mutants"), "gcs_math.h", MUTANTS, os.path.join(HERE, "hostemu", "wg_emu.cpp"))


def _run(oracle_lib, lib, name, cold):
    g = load_fixture(name)[1]
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL, warm_start=not cold)
    warm = None if cold else WarmRecords(lib, g)
    mode = "cold" if cold else "warm"
    agree, newton = Agreement(f"{name} {mode}"), NewtonParity(f"{name} {mode}")
    for it in range(STEPS):
        a = wg_step(lib, "wg_emu_vertex_step", g, o.zedge.copy(), o.mu.copy(), warm=warm)
        fails, iters, per_vertex = oracle_step(o)
        gen = a[5]
        agree.add(g, gen, a[0], a[3], o.copy, o.yv)
        newton.add(a[4][1], iters, a[4][0], fails, a[7][gen], per_vertex[gen])
        o.edge_step(1.0)
    return agree, newton


@pytest.mark.parametrize("name", ["benchmark4", "benchmark1"])
def test_clean_copy_meets_the_contract(builds, oracle_lib, name):
    for cold in (False, True):
        agree, newton = _run(oracle_lib, builds["clean"], name, cold)
        assert agree.legacy_ok()
        agree.check()
        newton.check(cold)


@pytest.mark.parametrize("mutant", ["reg_delta", "centring"])
@pytest.mark.parametrize("name", ["benchmark4", "benchmark1"])
def test_legacy_statistic_passes_what_the_contract_rejects(builds, oracle_lib, name, mutant):
    agree, _ = _run(oracle_lib, builds[mutant], name, cold=False)
    print(agree.summary())
    assert agree.legacy_ok(), "the seeded error should pass the legacy statistic (it is the reason the contract exists)"
    assert agree.failures(), "the contract let a seeded error through:\n" + agree.summary()


@pytest.mark.parametrize("name", ["benchmark4", "benchmark1"])
def test_newton_parity_rejects_a_perturbed_scaling(builds, oracle_lib, name):
    for cold in (False, True):
        _, newton = _run(oracle_lib, builds["eta"], name, cold)
        with pytest.raises(AssertionError):
            newton.check(cold)
