"""Edits of a decided scene on the device (gcsadmm_scene_add_regions / gcsadmm_scene_remove_regions in csrc/polytope_lp.hip through
scene.DeviceScene and queries.SceneQueries): after every edit everything the scene holds equals, bit for bit, what a scene built from
scratch on the edited list of regions holds; locate and restrict_paths see the edited regions; refused edits change nothing.  The host
build of the same code runs the box cases of test_scene_edit.py."""
import numpy as np
import pytest

import restrict_cases as R
import sweep_cases as S
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError

pytestmark = pytest.mark.gpu

FIELDS = ("cen", "rad", "st_c", "lo", "hi", "st_b", "pa", "pb", "flags", "st_o")


def decided(polys, tol=1e-9):
    """a scene with its graph decided (the caller closes it)"""
    scene = sc.DeviceScene(polys)
    scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps(tol)
    return scene


def state(scene):
    """everything a decided scene holds, read back without running an LP"""
    return dict(zip(FIELDS, scene.regions() + scene.pairs()))


_scratch = {}


def from_scratch(label, polys):
    """the state of a scene built from scratch on ``polys``, computed once per (label, length); no LP of it may report status < 0, so
    that no comparison hides behind an undecided pair"""
    key = (label, len(polys))
    if key not in _scratch:
        with decided(polys) as scene:
            _scratch[key] = state(scene)
        ref = _scratch[key]
        assert np.all(ref["st_c"] >= 0) and np.all(ref["st_b"] >= 0) and np.all(ref["st_o"] >= 0), key
        assert np.all(ref["rad"] > 0)
    return _scratch[key]


def assert_same(got, ref, what):
    for f in FIELDS:
        a, b = np.asarray(got[f]), np.asarray(ref[f])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, f)


def box_polys(lo, hi):
    n = lo.shape[1]
    A = np.vstack([np.eye(n), -np.eye(n)])
    return [(A, np.hstack([h, -l])) for l, h in zip(lo, hi)]


def region_list(name):
    if name == "benchmark4":
        from gcs_admm_amd.cases import fixture_sets
        As, bs, _, _, _ = fixture_sets(name)
        return [(np.asarray(As[k], float), np.asarray(bs[k], float)) for k in As if k not in ('s', 't')]
    if name == "lattice":
        from gcs_admm_amd.graph import lattice_boxes
        g = lattice_boxes(6, 6)
        return [(g.poly_A[g.poly_ptr[i]:g.poly_ptr[i + 1]], g.poly_b[g.poly_ptr[i]:g.poly_ptr[i + 1]]) for i in range(g.num_vertices)]
    if name == "boxes200":
        return box_polys(*S.boxes(2, 200))
    import lp_cases
    return list(lp_cases.family("mixed_rows", int(name[len("mixed_rows"):])).polys)


# (regions, size of the prefix, sizes of the calls that add the rest); boxes200 has the call with K > 128
ADD_CASES = [("benchmark4", 25, (15,)), ("benchmark4", 1, (20, 19)), ("lattice", 20, (1, 7, 10)), ("boxes200", 60, (140,)),
             ("mixed_rows1", 100, (30,)), ("mixed_rows3", 64, (65, 1)), ("mixed_rows8", 127, (1, 1, 1))]


@pytest.mark.parametrize("name,prefix,calls", ADD_CASES)
def test_add_equals_a_scene_built_from_scratch(name, prefix, calls):
    polys = region_list(name)
    assert prefix + sum(calls) == len(polys)
    with decided(polys[:prefix]) as scene:
        assert_same(state(scene), from_scratch(name, polys[:prefix]), "prefix")
        P = prefix
        for K in calls:
            before = scene.num_pairs
            cen, rad, st, counts = scene.add_regions(polys[P:P + K])
            P += K
            ref = from_scratch(name, polys[:P])
            assert scene.P == P and scene.num_pairs == len(ref["pa"])
            assert_same(state(scene), ref, (name, P))
            assert cen.tobytes() == ref["cen"][P - K:].tobytes() and rad.tobytes() == ref["rad"][P - K:].tobytes()
            assert np.array_equal(st, ref["st_c"][P - K:])
            new = ref["pb"] >= P - K                         # the LPs this call ran: its pairs are those with a new region
            assert counts == dict(new_pairs=int(new.sum()), overlapping=int(ref["flags"][new].sum()), undecided=0)
            assert counts["new_pairs"] == scene.num_pairs - before
        assert len(ref["pa"]) > 0 and 0 < int(ref["flags"].sum())


def test_add_nothing_changes_nothing():
    polys = region_list("lattice")
    with decided(polys) as scene:
        cen, rad, st, counts = scene.add_regions([])
        assert cen.shape == (0, 2) and counts == dict(new_pairs=0, overlapping=0, undecided=0)
        assert_same(state(scene), from_scratch("lattice", polys), "K = 0")


REMOVALS = {"first": lambda P: [0], "last": lambda P: [P - 1], "every_second": lambda P: list(range(0, P, 2)),
            "scattered": lambda P: [P - 2, 3, P // 2], "all_but_one": lambda P: [p for p in range(P) if p != 5][::-1]}


@pytest.mark.parametrize("what", sorted(REMOVALS))
@pytest.mark.parametrize("name", ["benchmark4", "mixed_rows3", "boxes200"])
def test_remove_equals_a_scene_built_from_scratch(name, what):
    polys = region_list(name)
    gone = REMOVALS[what](len(polys))
    left = [p for i, p in enumerate(polys) if i not in set(gone)]
    with decided(polys) as scene:
        assert scene.remove_regions(gone) == scene.num_pairs
        assert scene.P == len(left)
        with decided(left) as fresh:                         # (not cached: one list per case)
            ref = state(fresh)
        assert np.all(ref["st_o"] >= 0)
        assert_same(state(scene), ref, (name, what))


def test_remove_then_add_back_the_last_regions():
    for name in ("benchmark4", "mixed_rows8"):
        polys = region_list(name)
        P = len(polys)
        with decided(polys) as scene:
            scene.remove_regions(list(range(P - 7, P)))
            assert_same(state(scene), from_scratch(name, polys[:P - 7]), "removed")
            scene.add_regions(polys[P - 7:])
            assert_same(state(scene), from_scratch(name, polys), "added back")
            scene.remove_regions([])
            assert_same(state(scene), from_scratch(name, polys), "removed none")


def test_remove_from_a_scene_in_any_state():
    polys = region_list("benchmark4")
    left = polys[:3] + polys[5:]
    with sc.DeviceScene(polys) as scene:                     # nothing has run: the polytopes alone are compacted
        assert scene.remove_regions([3, 4]) == 0
        scene.centers(); scene.bounds()
        scene.remove_regions([0])                            # centres and boxes, no pairs
        scene.candidate_pairs(); scene.overlaps()
        assert_same(state(scene), from_scratch("benchmark4-left", left[1:]), "removed before the pairs")
    with sc.DeviceScene(polys) as scene:                     # pairs that are not decided yet
        scene.centers(); scene.bounds(); scene.candidate_pairs()
        scene.remove_regions([3, 4])
        ref = from_scratch("benchmark4-left2", left)
        pa, pb, flags, st = scene.pairs()
        assert flags is None and np.array_equal(pa, ref["pa"]) and np.array_equal(pb, ref["pb"])
        scene.overlaps()
        assert_same(state(scene), ref, "removed before the overlaps")


# ------------------------------------------------------------------------------------------- the other calls see the edited scene
def test_locate_and_restrict_paths_after_edits():
    _, n, polys, _, _ = R.corridor(6, 2)                     # six boxes in a row, each meeting the next
    centre = lambda p: 0.5 * (p[1][:n] - p[1][n:])
    with decided(polys[:4]) as scene, decided(polys) as whole, decided(polys[1:]) as tail:
        # added regions 4 and 5: a point inside 5 alone, one inside 4 and 5, one inside 0
        scene.add_regions(polys[4:])
        pts = np.array([centre(polys[5]) + [0.3, 0.0], 0.5 * (centre(polys[4]) + centre(polys[5])), centre(polys[0]) - [0.3, 0.0]])
        got, ref = scene.locate(pts), whole.locate(pts)
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        hits = np.split(got[1], got[0][1:-1])
        assert hits[0].tolist() == [5] and hits[1].tolist() == [4, 5] and hits[2].tolist() == [0]
        path = [2, 3, 4, 5]
        start = R.host_start(polys, path)
        got, ref = scene.restrict_paths([path], [start]), whole.restrict_paths([path], [start])
        assert got[3].tolist() == [0] and np.isfinite(got[1][0]) and got[1][0] > 0
        assert got[0][0].tobytes() == ref[0][0].tobytes() and got[1].tobytes() == ref[1].tobytes()
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
        # removed region 0: every index shifts down by one
        scene.remove_regions([0])
        got, ref = scene.locate(pts), tail.locate(pts)
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        hits = np.split(got[1], got[0][1:-1])
        assert hits[0].tolist() == [4] and hits[1].tolist() == [3, 4] and hits[2].tolist() == []      # the removed one is never listed
        path = [1, 2, 3, 4]
        got, ref = scene.restrict_paths([path], [start]), tail.restrict_paths([path], [start])
        assert got[3].tolist() == [0]
        assert got[0][0].tobytes() == ref[0][0].tobytes() and got[1].tobytes() == ref[1].tobytes()
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
        # and it is the path it was before the removal, under its new indices
        assert got[1].tobytes() == whole.restrict_paths([[2, 3, 4, 5]], [start])[1].tobytes()


# ------------------------------------------------------------------------------------------- refusals
def test_refused_edits_leave_the_scene_as_it_was():
    polys = region_list("benchmark4")
    n = 2
    A = np.vstack([np.eye(n), -np.eye(n)])
    good = (A, np.array([1.0, 1.0, 0.0, 0.0]))
    flat = (A, np.array([1.0, 1.0, 0.0, -1.0]))              # 0 <= x <= 1, y = 1: no interior
    with sc.DeviceScene(polys) as scene:
        scene.centers(); scene.bounds(); scene.candidate_pairs()
        with pytest.raises(GcsAdmmError, match=r"not decided: call gcsadmm_scene_overlaps first.*status 1"):
            scene.add_regions([good])
        assert scene.P == len(polys)
    with sc.DeviceScene(polys) as scene:
        with pytest.raises(GcsAdmmError, match=r"no resident centres: call gcsadmm_scene_centers first.*status 1"):
            scene.add_regions([good])
    with decided(polys) as scene:
        ref = from_scratch("benchmark4", polys)
        refusals = [([(np.zeros((0, n)), np.zeros(0))], r"polytope without rows.*status 1"),
                    ([good, (np.vstack([A, np.zeros((1, n))]), np.array([1.0, 1.0, 0.0, 0.0, 1.0]))], r"zero facet normal.*status 1"),
                    ([good, flat], r"new region 1.*status 1")]               # (no interior, or a centre LP that says so by not converging)
        for new, text in refusals:
            with pytest.raises(GcsAdmmError, match=text) as err:
                scene.add_regions(new)
            assert scene.P == len(polys) and scene.num_pairs == len(ref["pa"])
            assert_same(state(scene), ref, text)
        cen, rad, st = err.value.results                     # the flat one: the caller can name it
        assert rad[0] > 0 and st[0] >= 0 and (rad[1] <= 0 or st[1] < 0) and np.allclose(cen[0], 0.5)
        for gone, text in (([len(polys)], "out of range"), ([-1], "out of range"), ([3, 7, 3], "given twice")):
            with pytest.raises(GcsAdmmError, match=text + r".*status 1"):
                scene.remove_regions(gone)
            assert scene.P == len(polys) and scene.num_pairs == len(ref["pa"])
            assert_same(state(scene), ref, text)
        scene.add_regions([good])                            # and it still takes an edit
        assert scene.P == len(polys) + 1


# ------------------------------------------------------------------------------------------- SceneQueries
def test_scene_queries_grows_into_the_whole_scene():
    import locate_cases as L
    from gcs_admm_amd import SceneQueries
    As, bs, n, _ = L.region_sets("benchmark4")
    keys = list(As)
    part = lambda ks: ({k: As[k] for k in ks}, {k: bs[k] for k in ks})
    with SceneQueries(*part(keys[:-5]), n) as sq, SceneQueries(As, bs, n) as ref:
        sq.add_regions(*part(keys[-5:]))
        assert sq.keys == ref.keys and sq.centers.tobytes() == ref.centers.tobytes()
        assert np.array_equal(sq.edge_tail, ref.edge_tail) and np.array_equal(sq.edge_head, ref.edge_head)
        assert sq.stats["edit_centre_lps"] == 5 and sq.stats["edit_bound_lps"] == 20 and sq.stats["edit_pair_lps"] > 0
        assert sq.stats["candidate_pairs"] == ref.stats["candidate_pairs"] and sq.stats["overlaps_redone_on_host"] == 0
        S_, G_ = ref.centers[[0, 37]], ref.centers[[39, 2]]  # the second query starts in an added region
        for g, h in zip(sq.graphs(S_, G_), ref.graphs(S_, G_)):
            for f in ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr"):
                assert np.array_equal(getattr(g, f), getattr(h, f)), f
            assert g.poly_A.tobytes() == h.poly_A.tobytes() and g.poly_b.tobytes() == h.poly_b.tobytes() and g.interior.tobytes() == h.interior.tobytes()
        a, b = sq.solve(S_[:1], G_[:1])[0], ref.solve(S_[:1], G_[:1])[0]
        assert (a["status"], a["iterations"]) == (b["status"], b["iterations"])
        assert np.float64(a["rounded_cost"]).tobytes() == np.float64(b["rounded_cost"]).tobytes() and np.isfinite(a["rounded_cost"])
        sq.remove_regions(keys[-5:])
        with SceneQueries(*part(keys[:-5]), n) as small:
            assert sq.keys == small.keys and sq.centers.tobytes() == small.centers.tobytes()
            assert np.array_equal(sq.edge_tail, small.edge_tail) and np.array_equal(sq.edge_head, small.edge_head)
