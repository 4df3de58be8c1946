"""The contract of tests/lp_cases.py has teeth: the host build of the per-lane LP solver (tests/hostemu/lp_emu.cpp) compiled from a
copy of csrc/polytope_lp_core.h with one seeded error each must fail it, and the clean copy must pass.
  * the stop on the complementarity loosened from 1e-11 to 1e-6: boxes too small, radii off;
  * 0.99 -> 0.5 in the step rule: still converges to the same answers, in more Newton steps than the bound allows;
  * the margin of the early dual bound dropped: touching regions 300 from the origin are decided "apart" on a dual bound that is
    only valid up to the dual residual times |x|."""
import pytest

import lp_cases as L
from mutant_build import build_mutants

# (anchor in polytope_lp_core.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "loose_stop": [("const double mu_stop = 1e-11 * fmax(", "const double mu_stop = 1e-6 * fmax(")],
    "short_steps": [("const double al = fmin(1.0, 0.99 * amax);", "const double al = fmin(1.0, 0.5 * amax);")],
    "no_margin": [("hl < -tol - 1e-6)", "hl < -tol)")],
}
CASES = [(name, n) for n in (1, 2, 3) for name in ("touching", "scales", "mixed_rows")]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    return build_mutants(tmp_path_factory.mktemp("lp_mutants"), "polytope_lp_core.h", MUTANTS, L.EMU_SRC)


def _violations(lib):
    out = {}
    for name, n in CASES:
        fam = L.family(name, n)
        try:
            L.check_contract(fam, L.produce(L.HostLP(lib, fam.polys), fam), L.reference(name, n), newton=True)
        except AssertionError as e:
            out[name, n] = str(e)
    return out


def test_clean_copy_meets_the_contract(builds):
    assert _violations(builds["clean"]) == {}


@pytest.mark.parametrize("mutant,what", [("loose_stop", "radius|too small|against"), ("short_steps", "Newton steps"), ("no_margin", "wrong decisions")])
def test_contract_rejects_the_seeded_error(builds, mutant, what):
    import re
    found = _violations(builds[mutant])
    print(found)
    assert found, f"the contract let the seeded error {mutant} through"
    assert any(re.search(what, msg) for msg in found.values()), found
