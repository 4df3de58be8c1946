"""The resident scene on the device (gcsadmm_scene_* in csrc/polytope_lp.hip through scene.DeviceScene): sweep_kernel against
``scene.candidate_pairs`` element for element, the error paths, and the resident pipeline against the host pipeline bit for bit.
The same boxes go through the host build of the sweep in test_scene_resident.py."""
import numpy as np
import pytest

import sweep_cases as S
from conftest import BENCHMARKS, SMALL
from gcs_admm_amd import scene as sc
from gcs_admm_amd.cases import fixture_sets, load_fixture

pytestmark = pytest.mark.gpu


def unit_boxes(n, P):
    """P polytopes in R^n for a scene whose boxes are set by hand (the sweep reads the boxes alone)"""
    A = np.vstack([np.eye(n), -np.eye(n)]); b = np.ones(2 * n)
    return [(A, b)] * P


def device_pairs(scene, lo, hi, pad):
    scene.set_boxes(lo, hi)
    T = scene.candidate_pairs(pad)
    pa, pb, flags, st = scene.pairs()
    assert len(pa) == len(pb) == T and flags is None and st is None
    return pa, pb


def same_list(scene, lo, hi, pad):
    pa, pb = device_pairs(scene, lo, hi, pad)
    ra, rb = sc.candidate_pairs(lo, hi, pad)
    assert pa.dtype == pb.dtype == np.int32
    assert np.array_equal(pa, ra) and np.array_equal(pb, rb), (len(pa), len(ra))
    qa, qb = device_pairs(scene, lo, hi, pad)                  # a second call returns the same arrays
    assert np.array_equal(qa, pa) and np.array_equal(qb, pb)
    return pa, pb


@pytest.mark.parametrize("P", S.SIZES)
@pytest.mark.parametrize("n", S.DIMS)
def test_sweep_kernel_equals_candidate_pairs(n, P):
    lo, hi = S.boxes(n, P)
    with sc.DeviceScene(unit_boxes(n, P)) as scene:
        for pad in S.pads():
            pa, _ = same_list(scene, lo, hi, pad)
            S.check_share(P, len(pa))


@pytest.mark.parametrize("pad_index", [0, 1])
def test_sweep_kernel_on_ties_infinities_and_touching_boxes(pad_index):
    pad = S.pads()[pad_index]
    lo, hi = S.extras(pad)
    with sc.DeviceScene(unit_boxes(2, 130)) as scene:
        pa, pb = same_list(scene, lo, hi, pad)
    S.check_share(130, len(pa))
    S.check_extras(pa, pb)


def test_sweep_kernel_nothing_and_everything():
    lo = np.arange(65, dtype=float)[:, None] * np.array([[2.0, 0.0]]); hi = lo + 1.0        # 65 pairwise disjoint boxes
    with sc.DeviceScene(unit_boxes(2, 65)) as scene:
        pa, pb = device_pairs(scene, lo, hi, sc.SWEEP_PAD)
        assert len(pa) == 0 and len(pb) == 0
    lo = np.zeros((2000, 3)); hi = np.ones((2000, 3))                                        # 2 000 identical boxes: every pair
    with sc.DeviceScene(unit_boxes(3, 2000)) as scene:
        pa, pb = device_pairs(scene, lo, hi, 0.0)
    ta, tb = np.triu_indices(2000, 1)
    assert len(pa) == 1_999_000 and np.array_equal(pa, ta) and np.array_equal(pb, tb)


def test_scene_errors():
    from gcs_admm_amd.solver import GcsAdmmError
    with sc.DeviceScene(unit_boxes(2, 3)) as scene:
        lo = np.zeros((3, 2)); hi = np.ones((3, 2))
        bad = lo.copy(); bad[1, 1] = np.nan
        with pytest.raises(GcsAdmmError, match=r"NaN or with lo > hi.*status 1"):
            scene.set_boxes(bad, hi)
        bad = lo.copy(); bad[2, 0] = 1.5
        with pytest.raises(GcsAdmmError, match=r"NaN or with lo > hi.*status 1"):
            scene.set_boxes(bad, hi)
        with pytest.raises(GcsAdmmError, match=r"no resident boxes.*status 1"):           # the refused boxes were not taken
            scene.candidate_pairs()
        with pytest.raises(GcsAdmmError, match=r"no resident centres.*status 1"):
            scene.bounds()
        scene.set_boxes(lo, hi)
        with pytest.raises(GcsAdmmError, match=r"no resident pairs"):
            scene.pairs()
        assert scene.candidate_pairs() == 3
        with pytest.raises(GcsAdmmError, match=r"no resident centres"):
            scene.overlaps(1e-9)
    with pytest.raises(GcsAdmmError, match="closed"):
        scene.centers()
    with pytest.raises(GcsAdmmError, match=r"n = 1\.\.8.*status 2"):
        sc.DeviceScene(unit_boxes(9, 1))


def host_pipeline(polys, tol=1e-9):
    """the four steps of build_graph_device on a PolytopeScene, every intermediate kept"""
    host = sc.PolytopeScene(polys)
    cen, rad, st_c = host.centers()
    lo, hi, st_b = host.bounds(cen)
    st = np.asarray(st_b).reshape(len(polys), -1, 2)
    lo = np.where(st[:, :, 0] < 0, -np.inf, lo); hi = np.where(st[:, :, 1] < 0, np.inf, hi)
    pa, pb = sc.candidate_pairs(lo, hi)
    flags, st_o = host.overlaps(pa, pb, tol, cen)
    return dict(cen=cen, rad=rad, st_c=st_c, lo=lo, hi=hi, st_b=st_b, pa=pa, pb=pb, flags=flags, st_o=st_o)


def resident_pipeline(polys, tol=1e-9):
    with sc.DeviceScene(polys) as scene:
        cen, rad, st_c = scene.centers()
        lo, hi, st_b = scene.bounds()
        T = scene.candidate_pairs()
        over, undecided = scene.overlaps(tol)
        pa, pb, flags, st_o = scene.pairs()
    assert T == len(pa) and over == int(flags.sum()) and undecided == int((st_o < 0).sum())
    return dict(cen=cen, rad=rad, st_c=st_c, lo=lo, hi=hi, st_b=st_b, pa=pa, pb=pb, flags=flags, st_o=st_o)


@pytest.mark.parametrize("name", SMALL + BENCHMARKS)
def test_resident_pipeline_equals_host_pipeline(name):
    """edges (order included) equal the committed fixture; every intermediate of the resident scene is bitwise the host path's: the
    same kernels on the same inputs, and a pair list that is the host sweep's element for element"""
    case, gref = load_fixture(name)
    As, bs, n, _, _ = fixture_sets(name)
    keys = list(As.keys())
    polys = [(As[k], bs[k]) for k in keys]
    h, r = host_pipeline(polys), resident_pipeline(polys)
    for f in h:
        a, b = np.asarray(h[f]), np.asarray(r[f])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    stats, stats_host = {}, {}
    V, E, _, _, cen = sc.build_graph_device(As, bs, broad_phase="device", stats=stats)
    assert V == case["keys"] and [list(e) for e in E] == case["edges"]
    assert cen.tobytes() == h["cen"].tobytes()
    sc.build_graph_device(As, bs, stats=stats_host)
    assert stats == stats_host and stats["candidate_pairs"] == len(h["pa"])
    g = sc.graph_from_sets_device(As, bs, n, broad_phase="device")
    for f in ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr"):
        assert np.array_equal(getattr(g, f), getattr(gref, f)), f


@pytest.mark.parametrize("n", range(1, 9))
def test_resident_pipeline_on_general_polytopes(n):
    """tests/lp_cases.py mixed_rows (130 polytopes with their own row counts, widths and offsets) at every instantiated dimension"""
    import lp_cases
    fam = lp_cases.family("mixed_rows", n)
    As = {p: A for p, (A, _) in enumerate(fam.polys)}
    bs = {p: b for p, (_, b) in enumerate(fam.polys)}
    s_host, s_dev = {}, {}
    _, E_host, _, _, cen_host = sc.build_graph_device(As, bs, stats=s_host)
    _, E_dev, _, _, cen_dev = sc.build_graph_device(As, bs, stats=s_dev, broad_phase="device")
    assert E_dev == E_host and len(E_dev) > 0
    assert cen_dev.tobytes() == cen_host.tobytes()
    assert s_dev == s_host
    assert s_dev["bounds_opened"] == 0 and s_dev["overlaps_redone_on_host"] == 0


def test_resident_pipeline_on_the_lattice_at_scale():
    """10 002-box lattice: exactly the edges the generator's interval test finds, from the 19 703 candidate pairs of the host sweep"""
    from gcs_admm_amd.graph import lattice_boxes
    gref = lattice_boxes(100, 100, seed=0)
    polys = [(gref.poly_A[gref.poly_ptr[i]:gref.poly_ptr[i + 1]], gref.poly_b[gref.poly_ptr[i]:gref.poly_ptr[i + 1]]) for i in range(gref.num_vertices)]
    stats = {}
    tail, head, _ = sc.build_graph_arrays_device(polys, stats=stats)
    assert tail.dtype == head.dtype == np.int32
    assert np.array_equal(tail, gref.edge_tail) and np.array_equal(head, gref.edge_head)
    assert stats == dict(bounds_opened=0, overlaps_redone_on_host=0, candidate_pairs=19703)
