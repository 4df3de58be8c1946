"""segment_clip_kernel and segment_chain_kernel on the device (gcsadmm_scene_clip_segments / read_hits / read_spans / read_cover through
scene.DeviceScene.clip_segments) against their host build byte for byte -- all nine arrays, divisions included -- on the families,
lattices and crafted cases of test_segment_clip.py, which holds that build to references of its own; the refusals, the kind of the
resident list, the locate and project calls around a clip call, and ``SceneQueries.path_cover`` end to end around an edit."""
import ctypes as C

import numpy as np
import pytest

import cover_cases as cc
import locate_box_cases as bxc
import locate_cases as L
import project_cases as pc
import replanning_cases as R
from gcs_admm_amd import abi, queries
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError
from test_segment_clip import check_crafted

pytestmark = pytest.mark.gpu


def same(got, want, what):
    assert len(got) == len(want) == len(cc.FIELDS)
    for g, w, f in zip(got, want, cc.FIELDS):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, f)


@pytest.mark.parametrize("n", L.DIMS)
@pytest.mark.parametrize("kind,offset", L.FAMILIES)
def test_kernels_equal_the_host_build(kind, offset, n):
    """the nine arrays equal the host build's for 1 and 12 segments (P = 600: the scan across three chunks), and a second call returns
    them again"""
    assert max(cc.SIZES) > 2 * L.CHUNK
    for P in cc.SIZES:
        polys, start, end, want = cc.family(kind, n, P, offset)
        with sc.DeviceScene(polys) as scene:
            same(scene.clip_segments(start[:1], end[:1]), cc.family(kind, n, P, offset, 1)[3], (P, 1))
            same(scene.clip_segments(start, end), want, (P, cc.Q))
            same(scene.clip_segments(start, end), want, (P, "second call"))


@pytest.mark.parametrize("rotate", [None, 7])
def test_lattices_with_a_hole_on_the_device(rotate):
    for n, offset in cc.LATTICES:
        polys, start, end, want = cc.lattice_case(n, offset, rotate)
        with sc.DeviceScene(polys) as scene:
            same(scene.clip_segments(start, end), want, (n, offset, rotate))
        assert (want[5] == cc.GAP).any() and (want[5] == cc.COVERED).any()


def test_crafted_cases_on_the_device():
    names, polys, start, end, expect = cc.crafted()
    with sc.DeviceScene(polys) as scene:
        res = scene.clip_segments(start, end)
        same(res, cc.emu_clip(polys, start, end), "crafted")
        check_crafted(res, names, polys, start, end, expect)
        for tol in (0.0, 1e-3):
            same(scene.clip_segments(start, end, tol), cc.emu_clip(polys, start, end, tol), ("tol", tol))
        empty = scene.clip_segments(np.zeros((0, 2)), np.zeros((0, 2)))                  # zero segments
        assert empty[0].tolist() == [0] and empty[7].tolist() == [0] and all(len(a) == 0 for a in empty[1:7] + empty[8:])
        nothing = scene.clip_segments(np.full((3, 2), 100.0), np.full((3, 2), 101.0))      # segments that meet no region: no list, three gaps at 0
        same(nothing, cc.emu_clip(polys, np.full((3, 2), 100.0), np.full((3, 2), 101.0)), "no hits")
        assert nothing[0].tolist() == [0, 0, 0, 0] and nothing[5].tolist() == [cc.GAP] * 3 and nothing[6].tolist() == [0.0] * 3
    polys, start, end = cc.collinear(130)                                               # a chain longer than a stride
    with sc.DeviceScene(polys) as scene:
        res = scene.clip_segments(start, end)
        same(res, cc.emu_clip(polys, start, end), "collinear")
        assert len(res[8]) == 130


def test_refusals_leave_the_list_and_the_other_calls_are_unchanged():
    polys = L.regions("polytopes", 2, 130)
    pts = L.points("polytopes", 2, 130)[:6]
    start, end = np.ascontiguousarray(pts[:5]), np.ascontiguousarray(pts[1:])
    rad = pc.radii(5)
    lo, hi = bxc.boxes("polytopes", 2, 130, 0.0, 5)
    nulls = (None,) * 4
    with sc.DeviceScene(polys) as scene:
        for name, args in (("gcsadmm_scene_read_spans", nulls[:2]), ("gcsadmm_scene_read_cover", nulls)):      # before any list
            with pytest.raises(GcsAdmmError, match=r"no resident hit list.*status 1"):
                scene._call(name, *args)
        points_before, boxes_before, project_before = scene.locate(start), scene.locate_boxes(lo, hi), scene.project(start, rad)
        for name, args in (("gcsadmm_scene_read_spans", nulls[:2]), ("gcsadmm_scene_read_cover", nulls)):      # on a project call's list
            with pytest.raises(GcsAdmmError, match=r"the resident hit list is not a clip call's.*status 1"):
                scene._call(name, *args)
        scene.locate(start)
        with pytest.raises(GcsAdmmError, match=r"the resident hit list is not a clip call's.*status 1"):      # on a locate call's
            scene._call("gcsadmm_scene_read_cover", *nulls)
        want = cc.emu_clip(polys, start, end)
        same(scene.clip_segments(start, end), want, "clip")
        with pytest.raises(GcsAdmmError, match=r"the resident hit list is a locate call's.*status 1"):          # no projections on a clip list
            scene._call("gcsadmm_scene_read_projections", *nulls)
        for value in (np.nan, np.inf, -np.inf):
            for which in (0, 1):
                bad = [start.copy(), end.copy()]
                bad[which][3, 1] = value
                with pytest.raises(GcsAdmmError, match=r"segment with a NaN or an inf coordinate.*status 1"):
                    scene.clip_segments(*bad)
        for tol in (-1e-12, np.nan, np.inf):
            with pytest.raises(GcsAdmmError, match=r"tol must be finite and non-negative.*status 1"):
                scene.clip_segments(start, end, tol)
        num, links = C.c_int64(-7), C.c_int64(-7)
        for args in ((-1, start.ctypes.data, end.ctypes.data), (5, None, end.ctypes.data), (5, start.ctypes.data, None)):
            with pytest.raises(GcsAdmmError, match=r"negative number of segments or null end points.*status 1"):
                scene._call("gcsadmm_scene_clip_segments", *args, 1e-9, C.addressof(num), C.addressof(links))
        assert num.value == -7 and links.value == -7
        # the refused calls took nothing: the list made before them is still there, with its spans and chains
        T, K = len(want[1]), len(want[8])
        got = (np.zeros(6, np.int64), np.zeros(T, np.int32), np.zeros(T, np.uint8), np.zeros(T), np.zeros(T), np.zeros(5, np.int32), np.zeros(5),
               np.zeros(6, np.int64), np.zeros(K, np.int32))
        scene._call("gcsadmm_scene_read_hits", *(a.ctypes.data for a in got[:3]))
        scene._call("gcsadmm_scene_read_spans", *(a.ctypes.data for a in got[3:5]))
        scene._call("gcsadmm_scene_read_cover", *(a.ctypes.data for a in got[5:]))
        same(got, want, "after the refusals")
        # locate, locate_boxes and project give after a clip call what they gave before it, and clip the same after each of them
        for call, before in ((lambda: scene.locate(start), points_before), (lambda: scene.locate_boxes(lo, hi), boxes_before),
                             (lambda: scene.project(start, rad), project_before)):
            for a, b in zip(call(), before):
                assert a.tobytes() == b.tobytes()
            same(scene.clip_segments(start, end), want, "clip after another call")
    lib = abi.load_library()
    assert lib.gcsadmm_scene_clip_segments(None, 0, None, None, 1e-9, None, None) == 1          # a null scene is a bad argument
    assert lib.gcsadmm_scene_read_spans(None, None, None) == 1 and lib.gcsadmm_scene_read_cover(None, None, None, None, None) == 1


def _exact_reach(polys, p, q):
    """(status, reach) of the greedy sweep in rational arithmetic over the exact spans of the regions relaxed by tol S_i, the inner
    regions of the contract: where the cover of the segment p -> q by ``polys`` ends"""
    spans = [cc.exact_span(A, b, p, q - p)[0] for A, b in polys]
    status, reach, _ = cc.sweep([s for s in spans if s is not None])
    return status, reach


def test_a_removed_region_opens_a_gap_in_the_rounded_path_and_adding_it_back_closes_it():
    """benchmark4's regions, one query solved: its rounded path is covered, by a corridor that is a subsequence of the path's regions.
    A region of the corridor that no other region replaces (the sweep over the call's own spans without it ends early) is removed:
    the same call reports a gap in the segment that crossed it, at the parameter where the remaining regions end -- within 1e-9 of the
    reach of the greedy sweep in rational arithmetic over the exact spans of the remaining regions, each relaxed by tol S_i.  With the
    region back the path is covered again."""
    from gcs_admm_amd import SceneQueries
    As, bs, n, _ = L.region_sets(R.NAME)
    ref = R.Scene()
    with SceneQueries(As, bs, n) as sq:
        rec, = sq.solve(ref.s[None], ref.t[None])
        assert np.isfinite(rec["rounded_cost"])
        line = queries.rounded_polyline(rec)
        regions = [v for v in queries.rounded_path(rec) if v not in ('s', 't')]
        cover, = sq.path_cover([line])
        print("path", regions, "corridor", cover["corridor"], "points", len(line))
        assert cover["covered"] and cover["gap"] is None and cover["adjacent"] and len(cover["breaks"]) == len(cover["corridor"]) - 1
        rest = iter(regions)
        assert all(r in rest for r in cover["corridor"]), "the corridor is no subsequence of the rounded path's regions"
        # which region to take out: of the corridor's regions the one without which the sweep over the spans of this call leaves its
        # first gap deepest inside a segment (the path then enters the gap from a region that stays, at a parameter well above 0)
        res = sq.scene.clip_segments(line[:-1], line[1:])
        hit_ptr, hit_region, _, t_in, t_out = res[:5]
        found = []
        for key in cover["corridor"]:
            r = sq.keys.index(key)
            for j in range(len(line) - 1):
                at = [t for t in range(hit_ptr[j], hit_ptr[j + 1]) if hit_region[t] != r]
                status, reach, _ = cc.sweep([(t_in[t], t_out[t]) for t in at])
                if status == cc.GAP:      # the first gap of the path without this region
                    found.append((reach, key, j))
                    break
        print("first gap without each region of the corridor (reach, region, segment)", found)
        assert found and max(f[0] for f in found) > 0.01, "no region of the corridor leaves a gap inside a segment"
        _, gone, segment = max(found, key=lambda f: f[0])
        sq.remove_regions([gone])
        try:
            after, = sq.path_cover([line])
            status, reach = _exact_reach(sq.polys, line[segment], line[segment + 1])
            print("removed", gone, "gap", after["gap"], "exact", float(reach))
            assert status == cc.GAP
            assert not after["covered"] and after["gap"]["segment"] == segment and gone not in after["corridor"]
            assert abs(cc.F(after["gap"]["t"]) - reach) <= cc.F(1e-9)
            assert np.array_equal(after["gap"]["point"], line[segment] + after["gap"]["t"] * (line[segment + 1] - line[segment]))
        finally:
            sq.add_regions({gone: As[gone]}, {gone: bs[gone]})
        again, = sq.path_cover([line])
        assert again["covered"] and again["corridor"] == cover["corridor"] and again["adjacent"]
