"""project_list_kernel and project_solve_kernel on the device (gcsadmm_scene_project_points / read_hits / read_projections through
scene.DeviceScene.project) against their host build byte for byte -- all seven arrays, divisions and square roots included -- on the
families, crafted cases and rotated cubes of test_point_project.py, which holds that build to references of its own; the refusals, the
stage behaviour, the locate calls around a project call, and ``SceneQueries.solve(outside="snap")`` end to end."""
import ctypes as C

import numpy as np
import pytest

import locate_box_cases as bxc
import locate_cases as L
import project_cases as pc
import rotated_cases
from gcs_admm_amd import abi
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError
from test_point_project import check_crafted

pytestmark = pytest.mark.gpu


def same(got, want, what):
    assert len(got) == len(want) == len(pc.FIELDS)
    for g, w, f in zip(got, want, pc.FIELDS):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, f)


@pytest.mark.parametrize("n", L.DIMS)
@pytest.mark.parametrize("kind,offset", L.FAMILIES)
def test_kernels_equal_the_host_build(kind, offset, n):
    """the seven arrays equal the host build's for 1 and 12 points (radii 0, 0.05, 0.5, inf in turn: P = 600 with an infinite radius is
    600 solves per point and the scan across chunks), and a second call returns them again"""
    assert max(pc.SIZES) > 2 * L.CHUNK
    for P in pc.SIZES:
        polys, pts, rad, want = pc.family(kind, n, P, offset)
        with sc.DeviceScene(polys) as scene:
            same(scene.project(pts[:1], rad[:1]), pc.family(kind, n, P, offset, 1)[3], (P, 1))
            same(scene.project(pts, rad), want, (P, pc.Q))
            same(scene.project(pts, rad), want, (P, "second call"))
        assert len(want[1]) >= 3 * P and not np.any(want[5] == pc.FAILED)


def test_crafted_cases_and_rotated_cubes_on_the_device():
    names, polys, pts, rad, expect = pc.crafted()
    with sc.DeviceScene(polys) as scene:
        res = scene.project(pts, rad)
        same(res, pc.emu_project(polys, pts, rad), "crafted")
        check_crafted(res, names, polys, pts, rad, expect)
        for k in (0, 1):      # the iteration limit: no step, one step
            same(scene.project(pts, rad, max_iter=k), pc.emu_project(polys, pts, rad, max_iter=k), ("max_iter", k))
        same(scene.project(pts), pc.emu_project(polys, pts), "null radius")            # +inf for every point
        empty = scene.project(np.zeros((0, 2)))                                          # zero points
        assert empty[0].tolist() == [0] and all(len(a) == 0 for a in empty[1:]) and empty[4].shape == (0, 2)
    polys, pts, rad, d = pc.beyond_case()
    with sc.DeviceScene(polys) as scene:
        res = scene.project(pts, rad)
        same(res, pc.emu_project(polys, pts, rad), "beyond")
        assert res[5].tolist() == [pc.BEYOND] and abs(res[3][0] - d) < 1e-15
    for n in (3, 5, 8):
        R = rotated_cases.rotation(n, 100 + n)
        polys = [(np.vstack([R, -R]), np.ones(2 * n))]
        pts = np.vstack([np.random.default_rng(n).normal(size=(10, n)) * 2.0, R.T @ np.full(n, 3.0), np.zeros(n)])
        with sc.DeviceScene(polys) as scene:
            res = scene.project(pts)
            same(res, pc.emu_project(polys, pts), ("rotated", n))
            want = (R.T @ np.clip(R @ pts.T, -1, 1)).T
            assert np.all(res[5] == pc.SOLVED) and np.allclose(res[4], want, rtol=0, atol=1e-13)


def test_refusals_leave_the_list_and_the_locate_calls_are_unchanged():
    polys = L.regions("polytopes", 2, 130)
    pts = L.points("polytopes", 2, 130)[:5]
    rad = pc.radii(5)
    lo, hi = bxc.boxes("polytopes", 2, 130, 0.0, 5)
    with sc.DeviceScene(polys) as scene:
        with pytest.raises(GcsAdmmError, match=r"no resident hit list.*status 1"):      # before any list
            scene._call("gcsadmm_scene_read_projections", None, None, None, None)
        points_before, boxes_before = scene.locate(pts), scene.locate_boxes(lo, hi)
        with pytest.raises(GcsAdmmError, match=r"the resident hit list is a locate call's.*status 1"):
            scene._call("gcsadmm_scene_read_projections", None, None, None, None)
        want = pc.emu_project(polys, pts, rad)
        same(scene.project(pts, rad), want, "project")
        for value in (np.nan, np.inf, -np.inf):
            bad = pts.copy(); bad[3, 1] = value
            with pytest.raises(GcsAdmmError, match=r"point with a NaN or an inf coordinate.*status 1"):
                scene.project(bad, rad)
        for value in (np.nan, -1e-9, -np.inf):
            bad = rad.copy(); bad[2] = value
            with pytest.raises(GcsAdmmError, match=r"radius of point 2 is NaN or negative.*status 1"):
                scene.project(pts, bad)
        with pytest.raises(GcsAdmmError, match=r"max_iter must not be negative.*status 1"):
            scene.project(pts, rad, max_iter=-1)
        num = C.c_int64(-7)
        for args in ((-1, pts.ctypes.data), (5, None)):
            with pytest.raises(GcsAdmmError, match=r"negative number of points or null points.*status 1"):
                scene._call("gcsadmm_scene_project_points", *args, rad.ctypes.data, 100, C.addressof(num))
        assert num.value == -7
        # the refused calls took nothing: the list made before them is still there, with its projections
        T = len(want[1])
        got = (np.zeros(6, np.int64), np.zeros(T, np.int32), np.zeros(T, np.uint8), np.zeros(T), np.zeros((T, 2)), np.zeros(T, np.int32), np.zeros(T, np.int32))
        scene._call("gcsadmm_scene_read_hits", *(a.ctypes.data for a in got[:3]))
        scene._call("gcsadmm_scene_read_projections", *(a.ctypes.data for a in got[3:]))
        same(got, want, "after the refusals")
        # the locate calls give after a project call what they gave before it, and project the same after them
        for a, b in zip(scene.locate(pts), points_before):
            assert a.tobytes() == b.tobytes()
        with pytest.raises(GcsAdmmError, match=r"the resident hit list is a locate call's.*status 1"):
            scene._call("gcsadmm_scene_read_projections", *(a.ctypes.data for a in got[3:]))
        same(scene.project(pts, rad), want, "project after locate")
        for a, b in zip(scene.locate_boxes(lo, hi), boxes_before):
            assert a.tobytes() == b.tobytes()
        same(scene.project(pts, rad), want, "project after locate_boxes")
    lib = abi.load_library()
    assert lib.gcsadmm_scene_project_points(None, 0, None, None, 100, None) == 1          # a null scene is a bad argument
    assert lib.gcsadmm_scene_read_projections(None, None, None, None, None) == 1


def test_an_edit_ends_the_list_and_the_new_regions_are_projected_onto():
    polys = L.regions("polytopes", 2, 40)
    more = L.regions("polytopes", 2, 45)[40:]      # (the same seed family: other regions of the same domain)
    pts = L.points("polytopes", 2, 40)[:4]
    with sc.DeviceScene(polys) as scene:
        scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps()
        same(scene.project(pts), pc.emu_project(polys, pts), "before")
        scene.add_regions(more)
        with pytest.raises(GcsAdmmError, match=r"no resident hit list.*status 1"):
            scene._call("gcsadmm_scene_read_hits", None, None, None)
        with pytest.raises(GcsAdmmError, match=r"no resident hit list.*status 1"):
            scene._call("gcsadmm_scene_read_projections", None, None, None, None)
        same(scene.project(pts), pc.emu_project(polys + more, pts), "after add_regions")
        scene.remove_regions([0, 41])
        left = [p for i, p in enumerate(polys + more) if i not in (0, 41)]
        same(scene.project(pts, 0.5), pc.emu_project(left, pts, np.full(4, 0.5)), "after remove_regions")


def _same_value(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same_value(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same_value(x, y) for x, y in zip(a, b))
    if a is None or b is None or isinstance(a, str):
        return a is b or a == b
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_solve_with_a_start_outside_the_cover():
    from gcs_admm_amd import SceneQueries
    As, bs, n, _ = L.region_sets("four_boxes")
    start, goal = np.array([[-0.05, 0.5]]), np.array([[2.5, 0.5]])
    with SceneQueries(As, bs, n) as sq:
        with pytest.raises(ValueError, match=r"^query 0: the start lies in no region$"):
            sq.solve(start, goal)
        (near, d, x), = sq.nearest_regions(start)
        assert near == 0 and abs(d - 0.05) < 1e-15 and x.tolist() == [0.0, 0.5] and sq.last["redone_on_host"] == 0
        snapped = sq.solve(start, goal, outside="snap")
        moved = sq.solve(x[None], goal)
        assert len(snapped) == len(moved) == 1
        for f in ("rounded_cost", "x_v_rounded", "y_v_rounded", "iterations", "status"):
            assert _same_value(snapped[0][f], moved[0][f]), f
        rec = snapped[0]["snapped"]
        assert rec["goal"] is None and moved[0]["snapped"] == dict(start=None, goal=None)
        assert rec["start"]["original"].tolist() == [-0.05, 0.5] and rec["start"]["point"].tolist() == [0.0, 0.5]
        assert rec["start"]["region"] == 0 and rec["start"]["distance"] == d
        assert np.isfinite(snapped[0]["rounded_cost"])
        with pytest.raises(ValueError, match=r"the start lies in no region, and no region is within 0.01 of it"):
            sq.solve(start, goal, outside="snap", snap_radius=0.01)
        # a second batch, pruned and assembled on the device: the replaced point is what every stage sees
        starts, goals = np.array([[-0.05, 0.5], [0.5, 0.5]]), np.array([[2.5, 0.5], [2.5, 1.04]])
        pruned = sq.solve(starts, goals, outside="snap", prune="informed", assemble="induced")
        plain = sq.solve(np.array([[0.0, 0.5], [0.5, 0.5]]), np.array([[2.5, 0.5], [2.5, 1.0]]), prune="informed", assemble="induced")
        for a, b in zip(pruned, plain):
            for f in ("rounded_cost", "x_v_rounded", "iterations", "informed_bound", "kept_regions"):
                assert _same_value(a[f], b[f]), f
            assert a["graph"].interior.tobytes() == b["graph"].interior.tobytes()
        assert pruned[0]["snapped"]["start"]["region"] == 0 and pruned[1]["snapped"]["goal"]["point"].tolist() == [2.5, 1.0]
        assert pruned[1]["snapped"]["start"] is None
