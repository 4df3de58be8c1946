"""The general-polytope cases of tests/restrict_cases.py add teeth: the host emulation (tests/hostemu/restrict_emu.cpp) built from a copy
of csrc/path_restrict_core.h with one seeded error each passes every case the suite had before them (exact_cases, point_cases,
mixed_rows_case: congruent axis-aligned boxes, n = 1, 2, 3, 8) and is rejected by the new ones; the clean copy passes both.
  * diagonal_facets: the facets contribute to the diagonal of the Newton blocks only.  For +-unit rows A' diag(lam / s) A is
    diagonal, so no box sees it; any rotated or randomly faceted region sends the solve to the iteration limit.
  * dims_4_to_7: the slack of a row leaves coordinate 3 out for N = 4..7, instantiations that no earlier case ran.  That is so
    wrong that the start points already count as outside (status 1) in every case at those n.
  * dims_4_to_7_small: the same coordinate enters the slack 1e-7 too small.  The solve converges, on regions that are a little
    off: the rows of the returned points (assert_points_feasible) catch it, in a few cases the cost does.  One bent chain near
    the origin, held to the host solver within twice the bound, lets it through.
  * half_the_rows: scene_row takes half of a point's rows for the first of its two regions.  Right whenever both regions have the
    same number of rows, and in mixed_rows_case it only swaps a redundant cut for another redundant row; regions of different row
    counts (a point next to a polytope, the bent chains) get rows of the wrong region.  Such a row index runs past the region, so
    every scene solved here ends in a region that no path uses: the copy reads wrong rows, never outside the arrays.

Not every error moves a cost.  RESTRICT_REG = 1e-4 in place of 1e-10 passes every case, old and new, and is kept here as such
(test_errors_the_contract_does_not_see): the regularised matrix only makes the Newton direction inexact, and the residuals the
method recomputes in every iteration correct that.  The contract holds the answers, not the way the iteration takes to them.  (An
error in the residual itself is another matter: 1e-3 relative in one component of the right-hand side of ``direction`` sends the
longer staircases of the old cases to status -1 already.)"""
import os

import numpy as np
import pytest

import restrict_cases as rc
from mutant_build import build_mutants

# (anchor in path_restrict_core.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "diagonal_facets": [("v += dd[r] * A[g + a] * A[g + c];", "v += a == c ? dd[r] * A[g + a] * A[g + c] : 0.0;")],
    "dims_4_to_7": [("a -= A[(size_t)g * N + c] * q[(size_t)c * NP + j];",
                     "{ if (N >= 4 && N <= 7 && c == 3) continue; a -= A[(size_t)g * N + c] * q[(size_t)c * NP + j]; }")],
    "dims_4_to_7_small": [("a -= A[(size_t)g * N + c] * q[(size_t)c * NP + j];",
                           "a -= (N >= 4 && N <= 7 && c == 3 ? 1.0 - 1e-7 : 1.0) * A[(size_t)g * N + c] * q[(size_t)c * NP + j];")],
    "half_the_rows": [("const int r = P.poly[j - 1], m1 = P.poly_ptr[r + 1] - P.poly_ptr[r];",
                       "const int r = P.poly[j - 1], m1 = j < P.k ? (P.rowp[j + 1] - P.rowp[j]) / 2 : P.poly_ptr[r + 1] - P.poly_ptr[r];")],
    "large_reg": [("constexpr double RESTRICT_REG = 1e-10;", "constexpr double RESTRICT_REG = 1e-4;")],
}
SEEN = ["diagonal_facets", "dims_4_to_7", "dims_4_to_7_small", "half_the_rows"]
UNSEEN = ["large_reg"]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    libs = build_mutants(tmp_path_factory.mktemp("restrict_mutants"), "path_restrict_core.h", MUTANTS, rc.SRC,
                         flags=["-I" + rc.CSRC, "-I" + os.path.join(rc.ROOT, "include")])
    for lib in libs.values():
        lib.restrict_emu_solve.argtypes = rc.emu().restrict_emu_solve.argtypes
    return libs


def old_cases():
    return rc.exact_cases() + rc.point_cases() + [rc.mixed_rows_case()]


def violations(lib, cases):
    """{label: what assert_solution says} for the cases the build misses; the host's cost is the reference where there is no exact one"""
    out = {}
    for case in cases:
        label, n, polys, path, exact = case
        A0, b0 = rc.box(np.full(n, 50.0))
        pad = (np.tile(A0, (64, 1)), np.tile(b0, 64))                                   # 128 n rows that no path uses, last in the scene
        ptr, A, b, pp, poly, start = rc.flatten(n, polys + [pad], [path], [rc.case_start(case)])
        num = 1
        pts = np.full_like(start, np.nan); cost = np.full(num, np.nan); its = np.full(num, -7, np.int32); st = np.full(num, -7, np.int32)
        code = lib.restrict_emu_solve(n, len(ptr) - 1, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, num, pp.ctypes.data, poly.ctypes.data,
                                      start.ctypes.data, rc.TOL, rc.MAX_ITER, 0, pts.ctypes.data, cost.ctypes.data, its.ctypes.data, st.ctypes.data)
        assert code == rc.OK
        try:
            if st[0] == 0:
                try:
                    rc.assert_points_feasible(polys, path, pts)
                except AssertionError as e:
                    raise AssertionError(f"rows violated by {e}")
            extra = 2.0 * np.sqrt(n) * 1e-6 if label.endswith("-points") else 0.0
            reference = rc.host_cost(polys, path, n) if exact is None else None
            rc.assert_solution(case, pts, float(cost[0]), int(its[0]), int(st[0]), reference=reference, extra=extra)
        except AssertionError as e:
            out[label] = str(e) or "points outside their rows"
    return out


def test_clean_copy_meets_the_contract(builds):
    assert violations(builds["clean"], old_cases() + rc.general_cases()) == {}


@pytest.mark.parametrize("mutant", SEEN)
def test_old_cases_let_the_seeded_error_through(builds, mutant):
    assert violations(builds[mutant], old_cases()) == {}


@pytest.mark.parametrize("mutant,families,share", [("diagonal_facets", ["moved", "line", "thin", "far", "reflection", "bent"], 0.9),
                                                   ("dims_4_to_7", ["moved", "line", "reflection", "bent"], 0.0),
                                                   ("dims_4_to_7_small", ["moved", "line", "reflection", "bent"], 0.0),
                                                   ("half_the_rows", ["line", "thin", "far", "bent"], 0.9)])
def test_new_cases_reject_the_seeded_error(builds, mutant, families, share):
    """every named family rejects the error in at least one case at n >= 2, and together in the share ``share`` of them (the method
    sometimes still converges on a wrong Newton matrix, at n = 2 above all); dims_4_to_7: in every case at n = 4..7, in no other;
    dims_4_to_7_small: the same but for the bent chains, and at least once per family by the rows of the returned points"""
    total = caught = 0
    for fam in families:
        cases = [c for c in rc.family(fam) if c[1] >= 2]
        found = violations(builds[mutant], cases)
        print(mutant, fam, f"{len(found)} of {len(cases)}", found)
        assert found, f"family {fam} let the seeded error {mutant} through"
        if mutant.startswith("dims_4_to_7"):
            at_those = {c[0] for c in cases if 4 <= c[1] <= 7}
            assert set(found) <= at_those and (set(found) == at_those or (mutant, fam) == ("dims_4_to_7_small", "bent")), sorted(found)
        if mutant == "dims_4_to_7_small":
            assert any(msg.startswith("rows violated") for msg in found.values()), found
        total += len(cases); caught += len(found)
    assert caught >= share * total, (caught, total)


@pytest.mark.parametrize("mutant", UNSEEN)
def test_errors_the_contract_does_not_see(builds, mutant):
    """an error that the iteration itself corrects: every cost, old and new, stays within its bound (the module docstring has the
    reason).  If this fails, the contract has grown a tooth: move the mutant to SEEN."""
    assert violations(builds[mutant], old_cases() + rc.general_cases()) == {}
