"""The polytope LPs of graph construction (csrc/polytope_lp.hip: Chebyshev centres, bounding boxes, one overlap LP per pair) held to HiGHS
at every n = 1..8, over row counts that differ lane by lane, over seven orders of magnitude of size, at the LDS limit and on touching
regions -- tests/lp_cases.py has the families and the one contract.  The host build of the per-lane solver (tests/hostemu/lp_emu.cpp)
meets the contract on the CPU, Newton counts included; the device kernels meet it on the GPU and agree with the host build LP by LP."""
import numpy as np
import pytest

import lp_cases as L
from lp_cases import PO

DIMS = list(range(1, 9))
CASES = [(name, n) for name in ("mixed_rows", "scales", "touching") for n in DIMS] + [("polygon_limit", 2)]


@pytest.fixture(scope="module")
def lp_emu():
    return L.load_lp_emu()


@pytest.fixture(scope="module")
def host(lp_emu):
    """what the host build produces for a family, computed once per (family, n)"""
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            fam = L.family(name, n)
            cache[name, n] = L.produce(L.HostLP(lp_emu, fam.polys), fam)
        return cache[name, n]
    return get


def _poisoned(cen):
    """a centres array with a NaN, a +inf or a -inf in every third row each"""
    bad = np.array(cen, copy=True)
    for p in range(len(bad)):
        if p % 4 < 3:
            bad[p, p % bad.shape[1]] = (np.nan, np.inf, -np.inf)[p % 4]
    return bad


# ------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name,n", CASES)
def test_host_build_meets_the_contract(host, name, n):
    fam, ref = L.family(name, n), L.reference(name, n)
    fig = L.check_contract(fam, host(name, n), ref, newton=True)
    print(name, n, fig)
    if name == "mixed_rows":       # the family is what it says: three wavefronts, rows differing lane by lane, about half the pairs overlap
        rows = np.array([len(b) for _, b in fam.polys])
        assert len(fam.polys) == 130 and len(set(rows.tolist())) >= min(8, 3 * n) and rows.max() <= 79
        assert 0.3 <= (ref.rstar > 0).mean() <= 0.7


@pytest.mark.parametrize("n", DIMS)
def test_non_finite_start_is_not_an_overlap_on_the_host(lp_emu, host, n):
    """a start point with a NaN or an inf in it is replaced by the least-squares start: the decisions are the known ones and, LP by
    LP, those of a call without start points (the parent answered status 1, flag 1 at iteration 0 for every such pair)"""
    fam = L.touching(n)
    h = L.HostLP(lp_emu, fam.polys)
    cen = host("touching", n).cen
    bad = _poisoned(cen)
    flags, st = h.overlaps(fam.pa, fam.pb, L.TOL, bad)
    hit = ~np.isfinite(bad[fam.pa]).all(axis=1)
    assert hit.sum() >= len(fam.pa) // 2
    assert np.array_equal(flags, fam.expected), (flags.tolist(), st.tolist())
    f0, s0 = host("touching", n).flags["none"]
    assert np.array_equal(st[hit], np.asarray(s0)[hit]) and np.array_equal(flags[hit], np.asarray(f0)[hit])
    assert np.all(np.isfinite(h.r_o[st >= 0]))


def test_non_finite_result_has_no_status(lp_emu):
    """a bounds LP started from a non-finite centre, or from one outside its polytope, reports -1 and never a status >= 0"""
    fam = L.touching(3)
    h = L.HostLP(lp_emu, fam.polys)
    cen = h.centers()[0]
    bad = _poisoned(cen)
    bad[3] = cen[3] + 5.0                                        # finite, but outside the unit box 3
    lo, hi, st = h.bounds(bad)
    hit = ~np.isfinite(bad).all(axis=1); hit[3] = True
    assert np.all(st[hit] == -1) and np.all(st[~hit] == 0)
    assert np.all(np.isfinite(lo[~hit])) and np.all(np.isfinite(hi[~hit]))


# ------------------------------------------------------------------------------------------- GPU
def _scene(polys):
    from gcs_admm_amd.scene import PolytopeScene
    return PolytopeScene(polys)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [c for c in CASES if c[0] != "polygon_limit"])
def test_device_meets_the_contract_and_the_host_build(host, name, n):
    """ball_kernel<N> and bounds_kernel<N> through PolytopeScene.centers / bounds / overlaps: the contract against HiGHS, and statuses,
    flags, radii and boxes against the host build on the same inputs"""
    fam, ref = L.family(name, n), L.reference(name, n)
    dev = L.produce(_scene(fam.polys), fam)
    fig = L.check_contract(fam, dev, ref, newton=False)
    print(name, n, fig)
    L.check_against_host(fam, dev, host(name, n))


def _sub(fam, keep):
    """the polytopes `keep` of a family and the pairs among them"""
    idx = {p: i for i, p in enumerate(keep)}
    sel = [t for t in range(len(fam.pa)) if fam.pa[t] in idx and fam.pb[t] in idx]
    return L.Family(fam.name, fam.n, [fam.polys[p] for p in keep], fam.width[keep], np.array([idx[fam.pa[t]] for t in sel], np.int32),
                    np.array([idx[fam.pb[t]] for t in sel], np.int32), expected=fam.expected[sel], starts=fam.starts,
                    analytic={idx[p]: fam.analytic[p] for p in keep})


@pytest.mark.gpu
def test_device_at_the_lds_limit(lp_emu, host):
    """79 rows per polytope (overlaps) and 159 (centres) are the most that fit LDS: accepted and correct.  So is the largest row count
    the bounds launch admits (the launchers' own test, exported by the host build).  One row more is refused through the ABI with
    GCSADMM_ERR_UNSUPPORTED, "too many facet rows" -- a documented refusal, not a fault."""
    from gcs_admm_amd.solver import GcsAdmmError
    fam, ref = L.polygon_limit(), L.reference("polygon_limit", 2)
    m_c, m_o, m_b = (lp_emu.lp_emu_rows_admitted(k, 2) for k in range(3))
    assert (m_o, m_c) == L.POLYGON_SIDES and m_b < m_c
    # the 79-gons: all three LP kinds
    keep = [0, 1, 2]
    f79 = _sub(fam, keep)
    dev = L.produce(_scene(f79.polys), f79)
    r79 = L.Reference(ref.radius[keep], ref.lo[keep], ref.hi[keep], None)
    L.check_contract(f79, dev, r79, newton=False)
    h = host("polygon_limit", 2)
    assert np.array_equal(dev.flags["centres"][0], np.asarray(h.flags["centres"][0])[:len(f79.pa)])
    # the 159-gons: centres
    cen, rad, st = _scene(fam.polys).centers()
    assert np.all(st == 0) and np.abs(rad - 1.0).max() <= 1e-9 + 1e-11
    assert np.abs(cen - np.array([fam.analytic[p][0] for p in range(len(fam.polys))])).max() <= 1e-4     # sqrt(2 * 1e-9): the ball of radius 1 - 1e-9 pins its centre to that
    assert np.abs(rad - h.rad).max() <= 1e-9
    # the largest polygon the bounds launch takes
    A, b, lo_a, hi_a = L.regular_polygon(m_b, np.array([3.0, -2.0]))
    sc = _scene([(A, b)])
    lo, hi, st = sc.bounds(sc.centers()[0])
    assert np.all(st == 0)
    assert max((lo[0] - lo_a).max(), (hi_a - hi[0]).max()) <= L.BOX_SHORTFALL
    assert np.all(np.abs(lo[0] - lo_a) <= 1e-8 * np.maximum(1.0, np.abs(lo_a))) and np.all(np.abs(hi[0] - hi_a) <= 1e-8 * np.maximum(1.0, np.abs(hi_a)))
    # one row more
    for m, call in ((m_b + 1, lambda s: s.bounds(np.array([[3.0, -2.0]]))), (m_c + 1, lambda s: s.centers()),
                    (m_o + 1, lambda s: s.overlaps([0], [1], L.TOL, np.array([[3.0, -2.0], [3.0, -2.0]])))):
        poly = L.polygon_with_rows(m)
        with pytest.raises(GcsAdmmError, match=r"too many facet rows.*\(status 2\)"):
            call(_scene([poly, poly] if m == m_o + 1 else [poly]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS)
def test_device_non_finite_start_is_not_an_overlap(lp_emu, host, n):
    """gcsadmm_polytope_overlaps takes the start points from the caller: a NaN or an inf among them falls back to the least-squares
    start on the device as on the host build -- known answers, and the statuses of a call without start points"""
    fam = L.touching(n)
    sc = _scene(fam.polys)
    bad = _poisoned(host("touching", n).cen)
    flags, st = sc.overlaps(fam.pa, fam.pb, L.TOL, bad)
    assert np.array_equal(flags, fam.expected), (flags.tolist(), st.tolist())
    hit = ~np.isfinite(bad[fam.pa]).all(axis=1)
    sc._centers = None
    f0, s0 = sc.overlaps(fam.pa, fam.pb, L.TOL, None)
    assert np.array_equal(st[hit], s0[hit]) and np.array_equal(flags[hit], f0[hit])
    lo, hi, st_b = sc.bounds(bad)                                 # and a bounds LP from such a centre has no status >= 0
    assert np.all(st_b[~np.isfinite(bad).all(axis=1)] == -1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_device_batch_bounds_report_a_failed_side_and_open_nothing(n):
    """gcsadmm_polytope_bounds reports what the LPs left: started from a finite point outside polytope 3, every side of that polytope
    comes back with status -1 and lo == hi == the start coordinate (opening such a side is build_graph_arrays_device's job; the
    resident scene's bounds call opens it on the device), and every other side is bit for bit that of a call with the good centres"""
    fam = L.touching(n)
    sc = _scene(fam.polys)
    cen = sc.centers()[0]
    lo0, hi0, st0 = sc.bounds(cen)
    bad = np.array(cen, copy=True)
    bad[3] += 5.0
    lo, hi, st = sc.bounds(bad)
    print(n, st[3].tolist(), lo[3].tolist(), hi[3].tolist(), bad[3].tolist())
    assert st.shape == (len(fam.polys), 2 * n) and np.all(st[3] == -1)
    assert np.array_equal(lo[3], bad[3]) and np.array_equal(hi[3], bad[3])
    rest = np.arange(len(fam.polys)) != 3
    assert np.all(st[rest] == 0) and np.all(st0 == 0)
    assert np.array_equal(lo[rest], lo0[rest]) and np.array_equal(hi[rest], hi0[rest])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 5, 8])
def test_device_pipeline_on_mixed_rows(n):
    """centres -> boxes -> sweep -> pair LPs on 40 regions of the mixed_rows family: the edge list is the brute-force ordered double
    loop's (HiGHS feasibility per ordered pair), order included, and every decision was the device's"""
    from gcs_admm_amd.scene import build_graph_device
    fam = L.mixed_rows(n, P=40)
    As = {p: A for p, (A, _) in enumerate(fam.polys)}; bs = {p: b for p, (_, b) in enumerate(fam.polys)}
    stats = {}
    V, E, _, _, _ = build_graph_device(As, bs, stats=stats)
    ref = PO.edges(As, bs)
    assert [tuple(e) for e in E] == ref
    assert len(ref) >= 40
    assert stats["bounds_opened"] == 0 and stats["overlaps_redone_on_host"] == 0, stats


@pytest.mark.gpu
def test_device_pipeline_on_a_lattice_of_touching_boxes():
    """4 x 4 x 3 unit boxes sharing faces, edges and corners, 300 from the origin: the edges are those of the exact interval test
    (closed sets: every pair of cells at most one apart on every axis), found by the device from boxes that touch exactly"""
    from gcs_admm_amd.scene import build_graph_device
    cells = [(i, j, k) for i in range(4) for j in range(4) for k in range(3)]
    As = {c: L.box(300.0 + np.array(c), 301.0 + np.array(c))[0] for c in cells}
    bs = {c: L.box(300.0 + np.array(c), 301.0 + np.array(c))[1] for c in cells}
    stats = {}
    _, E, _, _, _ = build_graph_device(As, bs, stats=stats)
    ref = [(u, w) for u in cells for w in cells if u != w and max(abs(a - b) for a, b in zip(u, w)) <= 1]
    assert [tuple(e) for e in E] == ref
    assert stats["bounds_opened"] == 0 and stats["overlaps_redone_on_host"] == 0, stats
