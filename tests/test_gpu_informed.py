"""The informed region set of a query on the device (gcsadmm_scene_region_paths / _informed_regions in csrc/polytope_lp.hip through
scene.DeviceScene and queries.SceneQueries): the paths and the flags against the plain-numpy restatement of informed_cases.py, on the
scene's own centres, boxes and region graph as it reports them; the refusals; ``SceneQueries.informed`` with the device restriction
as the bound, and ``solve(prune="informed")`` end to end.  The host build of the same code runs the same cases without a device in
test_informed.py.  The tie rules are held vertex for vertex on ``lattice_twice``: a resident centre is the result of an LP, so the
integer lattice of the host build cannot be made resident, but regions with identical polytopes have bit-identical resident centres,
and every comparison between a cell and its copy ties exactly."""
import numpy as np
import pytest

import informed_cases as I
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError

gpu = pytest.mark.gpu

NEW_KERNELS = ("region_weight_kernel", "region_path_kernel", "informed_keep_kernel")


def test_new_kernels_use_no_scratch():
    """(no device needed: the compiler's resource remarks of the in-tree build)"""
    from gcs_admm_amd import build
    res = build.kernel_resources()
    for name in NEW_KERNELS:
        mine = {k: v for k, v in res.items() if name in k}
        assert len(mine) == 1, (name, sorted(mine))
        assert all(v["scratch"] == 0 for v in mine.values()), mine


def decided(c):
    """a scene of the case's boxes with its region graph built (the caller closes it), and what it holds: centres, lo, hi, row_ptr, tail,
    head"""
    scene = sc.DeviceScene(c.polys)
    scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps(1e-9)
    assert np.all(scene.pairs()[3] >= 0)
    scene.build_region_graph()
    cen, _, _, lo, hi, _ = scene.regions()
    row_ptr, tail, head, _ = scene.region_graph()
    assert np.array_equal(tail, c.tail) and np.array_equal(head, c.head) and np.array_equal(row_ptr, c.row_ptr)
    assert np.abs(lo - c.lo).max() < 1e-7 and np.abs(hi - c.hi).max() < 1e-7
    return scene, cen, lo, hi


# ------------------------------------------------------------------------------------------- search and keep
@gpu
@pytest.mark.parametrize("name", I.SCENES)
def test_paths_and_flags_equal_the_restatement(name):
    c = I.case(name)
    scene, cen, lo, hi = decided(c)
    with scene:
        w = I.weights(cen, c.tail, c.head)
        for B in I.BATCHES:
            pts, ptr, reg = c.batch(B)
            got = scene.region_paths(pts, ptr, reg)
            ref = I.check_paths(got, cen, c.row_ptr, c.tail, c.head, w, pts, ptr, reg)
            again = scene.region_paths(pts, ptr, reg)                  # the same on every run
            assert again[1].tobytes() == got[1].tobytes() and all(np.array_equal(a, b) for a, b in zip(again[0], got[0]))
            bound = np.array([r[1] if r[2] == 0 else 1.0 for r in ref])
            for scale in (1.0, 1.3, 0.5):
                I.check_keep(scene.informed_regions(pts, bound * scale), lo, hi, pts, bound * scale)
        pts, ptr, reg = c.batch(5)
        assert scene.informed_regions(pts, np.full(5, np.inf)).all()
        for pad in (0.0, 0.25):
            I.check_keep(scene.informed_regions(pts, bound, pad), lo, hi, pts, bound, pad)
        if name == "islands":
            assert list(got[2]) == [1, 1, 0, 0, 0]
        if name == "single":
            assert all(len(p) == 1 for p in got[0])
        if name == "boxes300":
            assert max(len(p) for p in got[0]) >= 20


@gpu
def test_identical_regions_tie_exactly_and_the_smaller_index_wins():
    """the goal rule (a cell and its copy lie under every goal), the step back (both explain every d) and the start test
    (``d[v] == init[v]``, the start distance computed a second time), as the device compiles them, vertex for vertex against the
    restatement on the centres the scene reports"""
    c = I.case("lattice_twice")
    scene, cen, _, _ = decided(c)
    with scene:
        assert cen[:48].tobytes() == cen[48:].tobytes()                 # what makes the ties exact
        w = I.weights(cen, c.tail, c.head)
        assert np.all(w[c.head == c.tail + 48] == 0.0) and np.count_nonzero(w == 0.0) == 96
        for B in I.BATCHES:
            pts, ptr, reg = c.batch(B)
            got = scene.region_paths(pts, ptr, reg)
            ref = I.check_paths(got, cen, c.row_ptr, c.tail, c.head, w, pts, ptr, reg, exact="paths")
            assert all(np.array_equal(d[:48], d[48:]) for _, _, _, d in ref)
            assert list(got[2]) == [0] * B and all(p.max() < 48 for p in got[0])
        assert all(set(r[r >= 48] - 48) == set(r[r < 48]) for r in np.split(reg, ptr[1:-1])) and max(len(p) for p in got[0]) >= 10
    whole = I.case("lattice")                                           # and the copies change no path
    scene, cen, _, _ = decided(whole)
    with scene:
        alone = scene.region_paths(*whole.batch(5))
        assert all(np.array_equal(p, q) for p, q in zip(got[0], alone[0])) and got[1].tobytes() == alone[1].tobytes()


@gpu
def test_max_len_is_reported_and_no_region_is():
    c = I.case("boxes300")
    scene, cen, _, _ = decided(c)
    with scene:
        pts, ptr, reg = c.batch(5)
        whole = scene.region_paths(pts, ptr, reg)
        paths, cost, status = scene.region_paths(pts, ptr, reg, max_len=7)
        assert [int(s) for s in status] == [0 if len(p) <= 7 else 2 for p in whole[0]] and 0 in status and 2 in status
        assert cost.tobytes() == whole[1].tobytes()
        assert all(np.array_equal(p, q) if s == 0 else len(p) == 0 for p, q, s in zip(paths, whole[0], status))


@gpu
def test_a_side_opened_to_infinity_never_counts():
    c = I.case("lattice")
    lo, hi = c.lo.copy(), c.hi.copy()
    lo[7, 0], hi[9, 1], lo[11], hi[11] = -np.inf, np.inf, -np.inf, np.inf
    pts, ptr, reg = c.batch(5)
    bound = np.array([2.0, 2.0, 5.0, 1.0, 1.0])
    with sc.DeviceScene(c.polys) as scene:
        scene.set_boxes(lo, hi)                                        # the boxes alone: the call needs nothing else
        got = scene.informed_regions(pts, bound)
        I.check_keep(got, lo, hi, pts, bound)
        scene.set_boxes(c.lo, c.hi)
        closed = scene.informed_regions(pts, bound)
        I.check_keep(closed, c.lo, c.hi, pts, bound)
        assert got[:, 11].all() and np.all(got >= closed) and np.any(got != closed)


# ------------------------------------------------------------------------------------------- refused input
@gpu
def test_refused_input_returns_its_status_and_changes_nothing():
    import re
    c = I.case("boxes2")
    pts, ptr, reg = c.batch(5)
    a_ = lambda x: None if x is None else x.ctypes.data
    with sc.DeviceScene(c.polys) as scene:
        with pytest.raises(GcsAdmmError, match=r"no resident boxes.*status 1"):
            scene.informed_regions(pts, np.ones(5))
        scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps(1e-9)
        with pytest.raises(GcsAdmmError, match=r"region graph.*status 1"):
            scene.region_paths(pts, ptr, reg)
        scene.build_region_graph()
        first = scene.region_paths(pts, ptr, reg)
        for label, text, kind, a in I.refusals(c.P, c.n, pts, ptr, reg):
            if kind == "paths":
                outs = [np.full((5, c.P), -3, np.int32), np.full(5, -3, np.int32), np.full(5, -3.0), np.full(5, -3, np.int32)]
                rc = scene.lib.gcsadmm_scene_region_paths(scene._h, a["B"], a_(a["pts"]), a_(a["ptr"]), a_(a["reg"]), a["max_len"], *(o.ctypes.data for o in outs))
            else:
                outs = [np.full((5, c.P), 7, np.uint8)]
                rc = scene.lib.gcsadmm_scene_informed_regions(scene._h, a["B"], a_(a["pts"]), a_(a["bound"]), a["pad"], outs[0].ctypes.data, None)
            assert rc == I.BAD_ARG, label
            assert re.search(text, scene.lib.gcsadmm_polytope_last_error().decode()), label
            assert all(np.all(o == (7 if kind == "keep" else -3)) for o in outs), label
        again = scene.region_paths(pts, ptr, reg)
        assert again[1].tobytes() == first[1].tobytes() and again[2].tobytes() == first[2].tobytes()
        none = scene.region_paths(np.zeros((0, 2)), np.zeros(1, np.int64), np.zeros(0, np.int32))
        assert none[0] == [] and scene.informed_regions(np.zeros((0, 2)), np.zeros(0)).shape == (0, c.P)
        outs = [np.full((5, c.P), -3, np.int32), np.full(5, -3, np.int32), np.full(5, -3.0), np.full(5, -3, np.int32)]
        empty = np.zeros(11, np.int64)                                   # queries without a hit, no hit array: no path each
        assert scene.lib.gcsadmm_scene_region_paths(scene._h, 5, pts.ctypes.data, empty.ctypes.data, None, c.P, *(o.ctypes.data for o in outs)) == I.OK
        assert np.all(outs[0] == -1) and np.all(outs[1] == 0) and np.all(np.isinf(outs[2])) and np.all(outs[3] == 1)
        # an edit ends the graph, and the paths with it; the boxes stay, and the keep call with them
        # the new region lies across the scene: rows grow and every edge id behind them moves -- weights kept from the graph before
        # the edit would show in the costs
        lo, hi = np.vstack([c.lo, [[1.0, 3.2]]]), np.vstack([c.hi, [[8.0, 3.8]]])
        scene.add_regions(I.box_polys(lo[-1:], hi[-1:]))
        with pytest.raises(GcsAdmmError, match=r"from before an edit.*status 1"):
            scene.region_paths(pts, ptr, reg)
        assert scene.informed_regions(pts, np.ones(5)).shape == (5, c.P + 1)
        scene.build_region_graph()
        row_ptr, tail, head, _ = scene.region_graph()
        want = I.region_graph_of(lo, hi)
        assert all(np.array_equal(a, b) for a, b in zip((row_ptr, tail, head), want)) and len(tail) >= len(c.tail) + 10
        cen = scene.regions()[0]
        ptr2, reg2 = I.term_lists(I.regions_under(lo, hi, pts))
        after = scene.region_paths(pts, ptr2, reg2)
        I.check_paths(after, cen, row_ptr, tail, head, I.weights(cen, tail, head), pts, ptr2, reg2)
        assert np.all(after[1] <= first[1] * (1 + 1e-12))                # (more edges: no path gets longer)


# ------------------------------------------------------------------------------------------- SceneQueries with the real bound
def lattice_queries():
    from gcs_admm_amd import SceneQueries
    c = I.case("lattice_wall")
    As = {("cell", r): A for r, (A, _) in enumerate(c.polys)}; bs = {("cell", r): b for r, (_, b) in enumerate(c.polys)}
    return c, SceneQueries(As, bs, 2)


@gpu
def test_informed_keeps_what_an_optimal_path_can_touch_and_solve_runs_on_it():
    c, sq = lattice_queries()
    with sq:
        S, G = c.S[:3], c.G[:3]                                          # two local queries and one across the scene
        info = sq.informed(S, G)
        regs = sq.regions_at(np.vstack([S, G]))
        for i, rec in enumerate(info):
            assert len(rec["path"]) >= 1 and np.linalg.norm(S[i] - G[i]) - 4e-6 <= rec["bound"] < np.inf
            inside = np.array([I.dist(S[i], m) + I.dist(m, G[i]) <= rec["bound"] for m in sq.centers])
            assert inside.any() and np.all(rec["keep"][inside])
            assert np.all(rec["keep"][regs[i]]) and np.all(rec["keep"][regs[3 + i]]) and np.all(rec["keep"][rec["path"]])
        whole = sq.solve(S, G)
        pruned = sq.solve(S, G, prune="informed")
        graphs = sq.graphs(S, G, prune="informed")
        for i, (rec, full) in enumerate(zip(pruned, whole)):
            assert "informed_bound" not in full and "kept_regions" not in full
            assert rec["informed_bound"] == info[i]["bound"] and rec["kept_regions"] == int(info[i]["keep"].sum())
            assert rec["rounded_cost"] <= rec["informed_bound"] * (1 + 1e-9)
            assert rec["graph"].num_vertices == 2 + rec["kept_regions"] == graphs[i].num_vertices
            assert rec["graph"].keys == ['s', 't'] + [sq.keys[r] for r in np.nonzero(info[i]["keep"])[0]]
            if full["rounded_cost"] <= rec["informed_bound"]:            # the unpruned answer lies inside the informed set
                on_path = [k for k, y in full["y_v_rounded"].items() if y and k not in ('s', 't')]
                assert on_path and all(info[i]["keep"][sq.keys.index(k)] for k in on_path)
        assert pruned[0]["kept_regions"] < c.P and pruned[1]["kept_regions"] < c.P      # the local queries run on a strict subset


@gpu
def test_the_informed_set_follows_an_edit():
    c, sq = lattice_queries()
    with sq:
        S, G = c.S[:2], c.G[:2]
        before = sq.informed(S, G)
        gone = [k for k, keep in zip(sq.keys, before[0]["keep"]) if not keep][:2]
        sq.remove_regions(gone)                                          # regions outside the first query's set: its path stays
        after = sq.informed(S, G)
        assert len(after[0]["keep"]) == c.P - 2 and after[0]["bound"] == pytest.approx(before[0]["bound"], rel=1e-9)
        assert [sq.keys[r] for r in after[0]["path"]] == [("cell", int(r)) for r in before[0]["path"]]
