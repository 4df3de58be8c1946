"""locate_kernel on the device (gcsadmm_scene_locate_points / read_hits through scene.DeviceScene.locate) against its host build element
for element, the error paths, and ``SceneQueries`` against from-scratch graph construction and solo solvers.  The same cases go through
the host build and the extended-precision restatement in test_point_locate.py."""
import ctypes as C

import numpy as np
import pytest

import locate_cases as L
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError
from gcs_admm_amd.graph import convert_pt_to_polytope

pytestmark = pytest.mark.gpu

INT_ARRAYS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr")


def same_hits(got, want, what):
    for g, w, f in zip(got, want, ("hit_ptr", "hit_region", "hit_class")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, f)


@pytest.mark.parametrize("n", L.DIMS)
@pytest.mark.parametrize("kind,offset", L.FAMILIES)
def test_locate_kernel_equals_the_host_build(kind, offset, n):
    """every P and Q of the family: the three arrays equal the host build's, and a second call returns them again"""
    for P in L.SIZES:
        pts = L.points(kind, n, P, offset)
        with sc.DeviceScene(L.regions(kind, n, P, offset)) as scene:
            for Q in L.QUERIES:
                want = L.family_hits(kind, n, P, offset, Q)
                same_hits(scene.locate(pts[:Q]), want, (P, Q))
                same_hits(scene.locate(pts[:Q]), want, (P, Q, "second call"))


def test_crafted_cases_on_the_device():
    names, polys, pts, expect = L.crafted(zero_rows=False)
    with sc.DeviceScene(polys) as scene:
        hits = scene.locate(pts)
        same_hits(hits, L.emu_locate(polys, pts), "crafted")
        L.check_crafted(hits, names, polys, pts, expect)
        assert all(len(h) == 0 for h in scene.locate(np.zeros((0, 2)))[1:]) and scene.locate(np.zeros((0, 2)))[0].tolist() == [0]      # Q = 0
    one = L.regions("boxes", 2, 1)                                                                                                  # P = 1
    inside = 0.5 * (one[0][1][:2] - one[0][1][2:])
    with sc.DeviceScene(one) as scene:
        hit_ptr, hit_region, hit_class = scene.locate([inside, inside + 100.0])
    assert hit_ptr.tolist() == [0, 1, 1] and hit_region.tolist() == [0] and hit_class.tolist() == [L.IN]
    # the regions with a row of zeros exist for the host build alone: a scene refuses them
    with pytest.raises(GcsAdmmError, match=r"zero facet normal.*status 1"):
        sc.DeviceScene(L.crafted()[1])


def test_argument_errors_leave_the_scene_as_it_was():
    polys, pts = L.regions("polytopes", 2, 130), L.points("polytopes", 2, 130)[:5]
    with sc.DeviceScene(polys) as scene:
        hit_ptr = np.zeros(6, np.int64)
        with pytest.raises(GcsAdmmError, match=r"no resident hit list.*status 1"):
            scene._call("gcsadmm_scene_read_hits", hit_ptr.ctypes.data, None, None)
        scene.centers(); scene.bounds()
        T = scene.candidate_pairs()
        counts = scene.overlaps()
        before = scene.pairs()
        assert T > 0 and counts[0] > 0
        want = L.emu_locate(polys, pts)
        same_hits(scene.locate(pts), want, "first")
        for bad in (np.nan, np.inf, -np.inf):
            q = pts.copy(); q[3, 1] = bad
            with pytest.raises(GcsAdmmError, match=r"NaN or an inf.*status 1"):
                scene.locate(q)
        for kw in (dict(eps=-1e-6), dict(tol=-1e-9), dict(eps=np.nan)):
            with pytest.raises(GcsAdmmError, match=r"eps and tol.*status 1"):
                scene.locate(pts, **kw)
        num = C.c_int64(-7)
        with pytest.raises(GcsAdmmError, match=r"negative number of points or null points.*status 1"):
            scene._call("gcsadmm_scene_locate_points", -1, pts.ctypes.data, 1e-6, 1e-9, C.addressof(num))
        with pytest.raises(GcsAdmmError, match=r"negative number of points or null points.*status 1"):
            scene._call("gcsadmm_scene_locate_points", 5, None, 1e-6, 1e-9, C.addressof(num))
        assert num.value == -7
        # the refused calls took nothing: the list made before them is still there, the pair list and its decisions are unchanged
        got = (np.zeros(6, np.int64), np.zeros(len(want[1]), np.int32), np.zeros(len(want[2]), np.uint8))
        scene._call("gcsadmm_scene_read_hits", *(a.ctypes.data for a in got))
        same_hits(got, want, "after the refusals")
        same_hits(scene.locate(pts), want, "again")
        after = scene.pairs()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert scene.overlaps() == counts and all(np.array_equal(a, b) for a, b in zip(before, scene.pairs()))
    from gcs_admm_amd import abi
    assert abi.load_library().gcsadmm_scene_locate_points(None, 0, None, 1e-6, 1e-9, None) == 1          # a null scene is a bad argument


# ------------------------------------------------------------------------------------------- query graphs against from-scratch builds
def benchmark3_queries():
    """(As, bs, n, starts [8, n], goals [8, n], what): deep points, one on a facet, one just beyond a vertex of polygon 15 where every
    row alone admits a point of the terminal's box and both together do not (104 degrees between rows 0 and 2, rotated against the
    axes; the point lies inside region 3)"""
    As, bs, n, _ = L.region_sets("benchmark3")
    rng = np.random.default_rng(3)
    keys = list(As)
    polys = [(np.asarray(As[k], float), np.asarray(bs[k], float)) for k in keys]
    from gcs_admm_amd.graph import chebyshev_center
    cen = np.array([chebyshev_center(A, b) for A, b in polys])
    deep = []
    while len(deep) < 14:
        r = int(rng.integers(len(polys)))
        p = cen[r] + rng.uniform(-0.3, 0.3, n)
        if np.all(polys[r][0] @ p <= polys[r][1]) and all(np.all(np.abs(A @ p - b) >= 1e-5 * np.abs(A).sum(axis=1)) for A, b in polys):
            deep.append(p)
    A15, b15 = polys[keys.index(15)]
    v = np.linalg.solve(A15[[0, 2]], b15[[0, 2]])
    unit = A15[[0, 2]] / np.linalg.norm(A15[[0, 2]], axis=1, keepdims=True)
    beyond = v + 1.5e-6 * unit.sum(axis=0) / np.linalg.norm(unit.sum(axis=0))
    A0, b0 = polys[0]
    t = (b0[0] - A0[0] @ cen[0]) / (A0[0] @ A0[0])
    facet = cen[0] + t * A0[0]                       # the foot of region 0's centre on its row 0 (it lies on that facet: the centre's
    assert np.all(A0[1:] @ facet < b0[1:] - 1e-3)    # ball touches there or stops short of it)
    S = np.array(deep[:8]); G = np.array(deep[8:] + [deep[0], deep[1]])
    S[1] = facet; G[2] = beyond
    return As, bs, n, S, G, dict(facet=(1, 's', 0), beyond=(2, 't', keys.index(15)))


def test_query_graphs_equal_from_scratch_builds():
    from gcs_admm_amd import SceneQueries
    As, bs, n, S, G, what = benchmark3_queries()
    with SceneQueries(As, bs, n) as sq:
        graphs = sq.graphs(S, G)
        last = dict(sq.last)
        centers = sq.centers.copy()
    assert len(graphs) == 8 and last["undecided"] >= 2 and last["redone_on_host"] == 0
    for i, g in enumerate(graphs):
        sets_A = {'s': convert_pt_to_polytope(S[i])[0], 't': convert_pt_to_polytope(G[i])[0], **As}
        sets_b = {'s': convert_pt_to_polytope(S[i])[1], 't': convert_pt_to_polytope(G[i])[1], **bs}
        ref = sc.graph_from_sets_device(sets_A, sets_b, n, broad_phase="device")
        assert g.keys == ref.keys and (g.src, g.dst, g.n) == (ref.src, ref.dst, ref.n)
        for f in INT_ARRAYS:
            a, b = getattr(g, f), getattr(ref, f)
            assert a.dtype == b.dtype and np.array_equal(a, b), (i, f)
        assert g.poly_A.tobytes() == ref.poly_A.tobytes() and g.poly_b.tobytes() == ref.poly_b.tobytes()
        assert g.interior[2:].tobytes() == ref.interior[2:].tobytes() == centers.tobytes(), i
        assert np.array_equal(g.interior[0], S[i]) and np.array_equal(g.interior[1], G[i])
    # the two special terminals were decided as the geometry says: on the facet the box meets the region, beyond the vertex it does not
    q, term, region = what["facet"]
    assert (0, region + 2) in set(zip(graphs[q].edge_tail.tolist(), graphs[q].edge_head.tolist()))
    q, term, region = what["beyond"]
    assert (1, region + 2) not in set(zip(graphs[q].edge_tail.tolist(), graphs[q].edge_head.tolist()))


# ------------------------------------------------------------------------------------------- end to end
def test_solve_equals_solo_solvers_and_the_reference_record():
    from gcs_admm_amd import SceneQueries
    from gcs_admm_amd.cases import fixture_sets, load_fixture
    from gcs_admm_amd.solver import DeviceSolver
    As_all, bs_all, n, _, _ = fixture_sets("benchmark1")
    case = load_fixture("benchmark1")[0]
    p = lambda k: (np.asarray(bs_all[k])[:n] - np.asarray(bs_all[k])[n:]) / 2
    As, bs, _, _ = L.region_sets("benchmark1")
    from gcs_admm_amd.graph import _as_box
    keys = list(As)

    def inner(k, f):                                                     # benchmark1's regions are boxes
        lo, hi = _as_box(np.asarray(As[k], float), np.asarray(bs[k], float))
        return lo + np.asarray(f) * (hi - lo)
    S = np.array([p('s'), inner(keys[0], (0.3, 0.6)), inner(keys[-1], (0.7, 0.2))])
    G = np.array([p('t'), inner(keys[-1], (0.4, 0.4)), inner(keys[1], (0.5, 0.5))])
    with SceneQueries(As, bs, n) as sq:
        records = sq.solve(S, G, return_state=True)
    assert len(records) == 3
    for i, rec in enumerate(records):
        solo = DeviceSolver(rec["graph"], "f64", device=0, program="workgroup256")
        want = solo.solve()
        assert (rec["status"], rec["iterations"]) == (want["status"], want["iterations"]), i
        assert rec["trace"].tobytes() == solo.trace.cpu().numpy().tobytes(), (i, "trace")
        for k, a in rec["state"].items():
            assert a.tobytes() == getattr(solo, k).cpu().numpy().tobytes(), (i, k)
        assert np.float64(rec["cost"]).tobytes() == np.float64(want["cost"]).tobytes()
        assert np.isfinite(rec["rounded_cost"]) and rec["y_v_rounded"]['s'] == 1 and rec["y_v_rounded"]['t'] == 1
        solo.close()
    # the fixture's own query: the committed graph, the reference's stop iteration and rounded length
    rec, gold = records[0], case["golden_v3"]
    assert rec["graph"].keys == case["keys"] and [list(e) for e in rec["graph"].edges_as_keys()] == case["edges"]
    assert rec["status"] == "converged" and rec["iterations"] == gold["iterations"] == 39
    x, y = rec["x_v_rounded"], rec["y_v_rounded"]
    length = sum(float(np.linalg.norm(np.asarray(x[v])[:n] - np.asarray(x[v])[n:])) for v in x if y[v] == 1)
    gx, gy = np.array(gold["x_v_rounded"]), np.array(gold["y_v_rounded"])
    glen = sum(np.linalg.norm(gx[i][:n] - gx[i][n:]) for i in range(len(gy)) if gy[i] == 1)
    assert abs(length - glen) <= 1e-5 * glen and abs(rec["rounded_cost"] - length) <= 1e-9 * glen
