"""The informed region set between start and goal SETS on the device (gcsadmm_scene_region_paths_sets / _informed_regions_sets in
csrc/polytope_lp.hip through scene.DeviceScene and queries.SceneQueries): on degenerate boxes the bits of the point calls on the same
resident scene; box terminals against the plain-numpy restatement of informed_set_cases.py, whose search runs to the end, on the
scene's own centres, boxes and region graph as it reports them; the refusals; and ``solve(prune="informed_sets")`` end to end.  The
host build of the same code runs the same cases without a device in test_informed_sets.py."""
import re

import numpy as np
import pytest

import informed_cases as I
import informed_set_cases as T
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError
from test_gpu_informed import decided, lattice_queries

gpu = pytest.mark.gpu

SCENES = ("lattice", "lattice_twice", "boxes3", "boxes300", "islands")


@gpu
@pytest.mark.parametrize("name", SCENES)
def test_degenerate_boxes_give_the_bits_of_the_point_calls(name):
    c = I.case(name)
    scene, _, _, _ = decided(c)
    with scene:
        pts, ptr, reg = c.batch(5)
        for first in ("sets", "points"):      # (the edge weights are made by whichever path call comes first)
            want = scene.region_paths(pts, ptr, reg) if first == "points" else None
            got = scene.region_paths_sets(pts, pts, ptr, reg)
            want = want or scene.region_paths(pts, ptr, reg)
            assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
            assert all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(got[0], want[0]))
        bound = np.where(want[2] == 0, want[1], 1.0)
        for scale, pad in ((1.0, sc.SWEEP_PAD), (1.3, 0.0), (0.5, 0.25)):
            assert np.array_equal(scene.informed_regions_sets(pts, pts, bound * scale, pad), scene.informed_regions(pts, bound * scale, pad))
        short = scene.region_paths_sets(pts, pts, ptr, reg, max_len=3), scene.region_paths(pts, ptr, reg, max_len=3)
        assert short[0][1].tobytes() == short[1][1].tobytes() and short[0][2].tobytes() == short[1][2].tobytes()


@gpu
@pytest.mark.parametrize("name", SCENES)
def test_box_terminals_equal_the_restatement(name):
    c = I.case(name)
    scene, cen, lo, hi = decided(c)
    with scene:
        w = I.weights(cen, c.tail, c.head)
        for kind, half in zip(T.KINDS, T.HALF_WIDTHS):
            tlo, thi, ptr, reg = T.batch(c, 5, kind, half)
            got = scene.region_paths_sets(tlo, thi, ptr, reg)
            ref = T.check_paths(got, cen, c.row_ptr, c.tail, c.head, w, tlo, thi, ptr, reg, exact=name == "lattice_twice")
            again = scene.region_paths_sets(tlo, thi, ptr, reg)            # the same on every run
            assert again[1].tobytes() == got[1].tobytes() and all(np.array_equal(a, b) for a, b in zip(again[0], got[0]))
            bound = np.array([r[1] if r[2] == 0 and r[1] > 0 else 1.0 for r in ref])
            for scale in (1.0, 1.3, 0.5):
                T.check_keep(scene.informed_regions_sets(tlo, thi, bound * scale), lo, hi, tlo, thi, bound * scale)
            T.check_keep(scene.informed_regions_sets(tlo, thi, bound, 0.25), lo, hi, tlo, thi, bound, 0.25)
        if name == "islands":
            assert list(got[2]) == [1, 1, 0, 0, 0]
        if name == "boxes300":                                             # lists longer than the 256 lanes
            tlo, thi, ptr, reg = T.wide_batch(c)
            got = scene.region_paths_sets(tlo, thi, ptr, reg)
            T.check_paths(got, cen, c.row_ptr, c.tail, c.head, w, tlo, thi, ptr, reg)
            again = scene.region_paths_sets(tlo, thi, ptr, reg)
            assert again[1].tobytes() == got[1].tobytes() and all(np.array_equal(a, b) for a, b in zip(again[0], got[0]))
            assert list(got[2]) == [0, 0] and len(got[0][0]) == 1
            bound = np.maximum(got[1], 0.5)
            T.check_keep(scene.informed_regions_sets(tlo, thi, bound), lo, hi, tlo, thi, bound)


@gpu
def test_refused_input_returns_its_status_and_changes_nothing():
    c = I.case("boxes2")
    tlo, thi, ptr, reg = T.batch(c, 5, "box_box", 0.3)
    a_ = lambda x: None if x is None else x.ctypes.data
    with sc.DeviceScene(c.polys) as scene:
        with pytest.raises(GcsAdmmError, match=r"no resident boxes.*status 1"):
            scene.informed_regions_sets(tlo, thi, np.ones(5))
        scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps(1e-9)
        with pytest.raises(GcsAdmmError, match=r"region graph.*status 1"):
            scene.region_paths_sets(tlo, thi, ptr, reg)
        scene.build_region_graph()
        first = scene.region_paths_sets(tlo, thi, ptr, reg)
        for label, text, kind, a in T.refusals(c.P, c.n, tlo, thi, ptr, reg):
            if kind == "paths":
                outs = [np.full((5, c.P), -3, np.int32), np.full(5, -3, np.int32), np.full(5, -3.0), np.full(5, -3, np.int32)]
                rc = scene.lib.gcsadmm_scene_region_paths_sets(scene._h, a["B"], a_(a["lo"]), a_(a["hi"]), a_(a["ptr"]), a_(a["reg"]), a["max_len"],
                                                               *(o.ctypes.data for o in outs))
            else:
                outs = [np.full((5, c.P), 7, np.uint8)]
                rc = scene.lib.gcsadmm_scene_informed_regions_sets(scene._h, a["B"], a_(a["lo"]), a_(a["hi"]), a_(a["bound"]), a["pad"], outs[0].ctypes.data, None)
            assert rc == I.BAD_ARG, label
            assert re.search(text, scene.lib.gcsadmm_polytope_last_error().decode()), label
            assert all(np.all(o == (7 if kind == "keep" else -3)) for o in outs), label
        again = scene.region_paths_sets(tlo, thi, ptr, reg)
        assert again[1].tobytes() == first[1].tobytes() and again[2].tobytes() == first[2].tobytes()
        none = np.zeros((0, 2))
        assert scene.region_paths_sets(none, none, np.zeros(1, np.int64), np.zeros(0, np.int32))[0] == []
        assert scene.informed_regions_sets(none, none, np.zeros(0)).shape == (0, c.P)
        # an edit ends the graph, and the paths with it, until the graph is rebuilt; the boxes stay, and the keep call with them
        lo, hi = np.vstack([c.lo, [[1.0, 3.2]]]), np.vstack([c.hi, [[8.0, 3.8]]])
        scene.add_regions(I.box_polys(lo[-1:], hi[-1:]))
        with pytest.raises(GcsAdmmError, match=r"from before an edit.*status 1"):
            scene.region_paths_sets(tlo, thi, ptr, reg)
        assert scene.informed_regions_sets(tlo, thi, np.ones(5)).shape == (5, c.P + 1)
        scene.build_region_graph()
        row_ptr, tail, head, _ = scene.region_graph()
        cen = scene.regions()[0]
        ptr2, reg2 = I.term_lists(T.meeting(lo, hi, tlo, thi))
        after = scene.region_paths_sets(tlo, thi, ptr2, reg2)
        T.check_paths(after, cen, row_ptr, tail, head, I.weights(cen, tail, head), tlo, thi, ptr2, reg2)
        assert np.all(after[1] <= first[1] * (1 + 1e-12))                # (more edges: no path gets longer)


@gpu
def test_solve_runs_box_queries_on_their_informed_sets():
    c, sq = lattice_queries()
    with sq:
        S, G = c.S[:3], c.G[:3]                                          # queries 0, 1 are local, 2 runs across the scene
        box = lambda pts: (pts - 0.3, pts + 0.3)
        queries = [(dict(starts=S[[0, 2]], goal_boxes=box(G[[0, 2]])), [0]),                 # point -> box: a local one and the one across
                   (dict(start_boxes=box(S[[1]]), goal_boxes=box(G[[1]])), [0])]             # box -> box: local
        for q, local in queries:
            info = sq.informed_sets(**q)
            pruned = sq.solve(prune="informed_sets", **q)
            whole = sq.solve(**q)
            graphs = sq.graphs(prune="informed_sets", assemble="induced", **q)
            for i, (rec, full) in enumerate(zip(pruned, whole)):
                assert "informed_bound" not in full and "kept_regions" not in full
                assert np.isfinite(rec["informed_bound"]) and rec["informed_bound"] == info[i]["bound"] and rec["kept_regions"] == int(info[i]["keep"].sum())
                assert rec["rounded_cost"] <= rec["informed_bound"] * (1 + 1e-9)
                assert rec["graph"].num_vertices == 2 + rec["kept_regions"] == graphs[i].num_vertices
                assert rec["graph"].keys == ['s', 't'] + [sq.keys[r] for r in np.nonzero(info[i]["keep"])[0]] == graphs[i].keys
                if full["rounded_cost"] <= rec["informed_bound"]:        # the unpruned answer lies inside the informed set
                    on_path = [k for k, y in full["y_v_rounded"].items() if y and k not in ('s', 't')]
                    assert on_path and all(info[i]["keep"][sq.keys.index(k)] for k in on_path)
            assert all(pruned[i]["kept_regions"] < c.P for i in local)      # the local queries run on a strict subset
