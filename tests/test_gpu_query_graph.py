"""The device assembly of query graphs on the device (gcsadmm_scene_build_region_graph / _read_region_graph / _query_graphs in
csrc/polytope_lp.hip through scene.DeviceScene and queries.SceneQueries): the region graph against ``scene.edge_arrays``, the query
graphs against the host build of the same code and against the host path, on the tables of query_graph_cases.py; the refusals;
``SceneQueries.graphs`` and ``solve`` with ``assemble="device"`` against ``assemble="host"``, bit for bit.  The host build of the same
code runs these tables without a device in test_query_graph.py."""
import numpy as np
import pytest

import locate_cases as L
import query_graph_cases as Q
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError

gpu = pytest.mark.gpu

NEW_KERNELS = ("region_count_kernel", "region_scatter_kernel", "region_place_kernel", "region_reverse_kernel", "query_graph_kernel")


def test_new_kernels_use_no_scratch():
    """(no device needed: the compiler's resource remarks of the in-tree build)"""
    from gcs_admm_amd import build
    res = build.kernel_resources()
    for name in NEW_KERNELS:
        mine = {k: v for k, v in res.items() if name in k}
        assert len(mine) == 1, (name, sorted(mine))
        assert all(v["scratch"] == 0 for v in mine.values()), mine


def decided(name):
    """a scene of boxes with its graph decided (the caller closes it), and its pair list"""
    scene = sc.DeviceScene(Q.box_polys(*Q.scene_boxes(name)))
    scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps(1e-9)
    pa, pb, flags, st = scene.pairs()
    assert np.all(st >= 0)
    return scene, pa, pb, flags


# ------------------------------------------------------------------------------------------- region graph
@gpu
@pytest.mark.parametrize("name", Q.SCENES)
def test_region_graph_equals_edge_arrays(name):
    scene, pa, pb, flags = decided(name)
    with scene:
        P = scene.P
        E = scene.build_region_graph()
        first = scene.region_graph()
        Q.check_region_graph(first, P, pa, pb, flags)
        assert E == len(first[1]) == 2 * int((flags != 0).sum())
        if name == "identical":
            assert E == 330 * 329
        if name == "hub":
            assert np.diff(first[0])[0] == 599
        if name == "apart":
            assert E == 0
        scene.build_region_graph()                                  # the same arrays on every run
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, scene.region_graph()))
        for density in Q.DENSITIES:                                 # host flags in the place of the resident ones
            host = Q.random_flags(len(pa), density)
            assert scene.build_region_graph(host) == 2 * int((host != 0).sum())
            Q.check_region_graph(scene.region_graph(), P, pa, pb, host)
        assert scene.pairs()[2].tobytes() == flags.tobytes()        # the resident flags stay
        scene.build_region_graph()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, scene.region_graph()))


# ------------------------------------------------------------------------------------------- query graphs
@gpu
@pytest.mark.parametrize("P", Q.REGIONS)
def test_query_graphs_equal_the_host_build_and_the_host_path(P):
    scene, pa, pb, _ = decided("boxes%d" % P)
    with scene:
        for density in Q.DENSITIES:
            flags = Q.random_flags(len(pa), density)
            scene.build_region_graph(flags)
            row_ptr, tail, head, _ = scene.region_graph()
            with Q.EmuGraph(P, pa, pb, flags) as emu:
                emu.build_region_graph()
                for B in Q.BATCHES:
                    term_ptr, term_region, st = Q.hit_lists(P, B, np.diff(row_ptr), seed=B)
                    runs = [scene.query_graphs(term_ptr, term_region, st, chunk) for chunk in Q.CHUNKS]
                    assert Q.same_bytes(runs[0], emu.query_graphs(term_ptr, term_region, st))
                    assert Q.same_bytes(runs[0], runs[1]) and Q.same_bytes(runs[0], runs[2])
                    if B <= 5:
                        Q.check_query_graphs(runs[0], tail, head, P, term_ptr, term_region, st)


@gpu
@pytest.mark.parametrize("name", ["identical", "hub", "apart"])
def test_query_graphs_on_the_extreme_degrees(name):
    scene, pa, pb, flags = decided(name)
    with scene:
        scene.build_region_graph()
        row_ptr, tail, head, _ = scene.region_graph()
        term_ptr, term_region, st = Q.hit_lists(scene.P, 5, np.diff(row_ptr))
        for chunk in (0, 3):
            Q.check_query_graphs(scene.query_graphs(term_ptr, term_region, st, chunk), tail, head, scene.P, term_ptr, term_region, st)
        empty = scene.query_graphs(np.array([0, 0, 0], np.int64), np.zeros(0, np.int32), np.array([1], np.uint8))      # no hit at all
        Q.check_query_graphs(empty, tail, head, scene.P, np.array([0, 0, 0], np.int64), np.zeros(0, np.int32), np.array([1], np.uint8))
        assert scene.query_graphs(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8)) == []


def _raw(scene, a, outs):
    ptr = lambda x: None if x is None else x.ctypes.data
    return scene.lib.gcsadmm_scene_query_graphs(scene._h, a["B"], ptr(a["ptr"]), ptr(a["reg"]), ptr(a["st"]), a["chunk"], ptr(a["off"]),
                                                *(o.ctypes.data for o in outs))


@gpu
def test_refused_input_returns_its_status_and_changes_nothing():
    import re
    scene, pa, pb, flags = decided("boxes130")
    with scene:
        P = scene.P
        with pytest.raises(GcsAdmmError, match=r"no resident region graph.*status 1"):
            scene.region_graph()
        E_R = scene.build_region_graph()
        graph = scene.region_graph()
        term_ptr, term_region, st = Q.hit_lists(P, 5, np.diff(graph[0]), seed=1)
        off = Q.edge_offsets(E_R, term_ptr, st)
        for label, status, text, a in Q.refusals(P, E_R, term_ptr, term_region, st):
            outs = Q.raw_outputs(5, P, int(off[-1]))
            assert _raw(scene, a, outs) == status, label
            assert re.search(text, scene.lib.gcsadmm_polytope_last_error().decode()), label
            assert all(np.all(o == -3) for o in outs), label
            assert all(x.tobytes() == y.tobytes() for x, y in zip(graph, scene.region_graph())), label
        ok = dict(B=5, ptr=term_ptr, reg=term_region, st=st, chunk=0, off=off)
        outs = Q.raw_outputs(5, P, int(off[-1]))
        assert _raw(scene, ok, outs) == Q.OK and not any(np.any(o == -3) for o in outs)
        with pytest.raises(ValueError, match="flags must be"):
            scene.build_region_graph(np.ones(len(pa) + 1, np.uint8))
    with sc.DeviceScene(Q.box_polys(*Q.scene_boxes("boxes65"))) as scene:       # pairs that are not decided yet
        scene.centers(); scene.bounds(); scene.candidate_pairs()
        with pytest.raises(GcsAdmmError, match=r"not decided: call gcsadmm_scene_overlaps first.*status 1"):
            scene.build_region_graph()


@gpu
def test_an_edit_ends_the_graph_and_a_rebuild_follows_it():
    lo, hi = Q.scene_boxes("boxes130")
    polys = Q.box_polys(lo, hi)
    scene = sc.DeviceScene(polys[:100])
    with scene:
        scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps(1e-9)
        scene.build_region_graph()
        ptr, reg, st = np.array([0, 1, 2], np.int64), np.array([3, 7], np.int32), np.array([0], np.uint8)
        before = scene.query_graphs(ptr, reg, st)
        edits = [lambda: scene.add_regions(polys[100:]), lambda: scene.remove_regions([0, 50, 129]), lambda: scene.overlaps(1e-9),
                 lambda: scene.candidate_pairs()]
        for k, edit in enumerate(edits):
            edit()
            for call in (lambda: scene.query_graphs(ptr, reg, st), scene.region_graph):
                with pytest.raises(GcsAdmmError, match=r"region graph.*status 1"):
                    call()
            if k == 3:
                scene.overlaps(1e-9)
            scene.build_region_graph()
            pa, pb, flags, _ = scene.pairs()
            row_ptr, tail, head, rev = scene.region_graph()
            Q.check_region_graph((row_ptr, tail, head, rev), scene.P, pa, pb, flags)
            Q.check_query_graphs(scene.query_graphs(ptr, reg, st), tail, head, scene.P, ptr, reg, st)
        assert scene.P == 127 and len(before[0][2]) == 103
        scene.add_regions([]); scene.remove_regions([])             # edits of nothing leave it
        assert len(scene.query_graphs(ptr, reg, st)) == 1


# ------------------------------------------------------------------------------------------- SceneQueries against its host path
FIELDS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr", "poly_A", "poly_b", "interior")


def assert_same_graphs(got, ref):
    assert len(got) == len(ref) > 0
    for g, h in zip(got, ref):
        assert (g.n, g.keys, g.src, g.dst) == (h.n, h.keys, h.src, h.dst)
        for f in FIELDS:
            a, b = getattr(g, f), getattr(h, f)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f


def _points(sq, count, seed=0):
    rng = np.random.default_rng(seed + len(sq.keys))
    return sq.centers[rng.integers(0, len(sq.keys), count)]


@gpu
@pytest.mark.parametrize("name", ["benchmark1", "benchmark2", "benchmark3", "benchmark4"])
def test_scene_queries_device_assembly_equals_the_host_path(name):
    from gcs_admm_amd import SceneQueries
    As, bs, n, _ = L.region_sets(name)
    with SceneQueries(As, bs, n) as sq:
        pts = _points(sq, 10)
        pts[5] = pts[0]                                             # start = goal
        assert_same_graphs(sq.graphs(pts[:5], pts[5:], assemble="device"), sq.graphs(pts[:5], pts[5:]))


def lattice_sets(nx, ny):
    from gcs_admm_amd.graph import lattice_boxes
    g = lattice_boxes(nx, ny)
    cells = range(2, g.num_vertices)
    return ({("cell", v - 2): g.poly_A[g.poly_ptr[v]:g.poly_ptr[v + 1]] for v in cells},
            {("cell", v - 2): g.poly_b[g.poly_ptr[v]:g.poly_ptr[v + 1]] for v in cells})


@gpu
def test_scene_queries_on_a_lattice_before_and_after_an_add_and_a_remove():
    from gcs_admm_amd import SceneQueries
    As, bs = lattice_sets(25, 40)
    keys = list(As)
    part = lambda ks: ({k: As[k] for k in ks}, {k: bs[k] for k in ks})
    with SceneQueries(*part(keys[:-30]), 2) as sq:
        def both(seed):
            pts = _points(sq, 16, seed)
            got = sq.graphs(pts[:8], pts[8:], assemble="device")
            assert_same_graphs(got, sq.graphs(pts[:8], pts[8:]))
            return got
        assert both(0)[0].num_vertices == 972
        sq.add_regions(*part(keys[-30:]))
        assert both(1)[0].num_vertices == 1002
        sq.remove_regions(keys[3:400:7])
        assert both(2)[0].num_vertices == 1002 - len(keys[3:400:7])
        assert sq.scene.num_region_edges == len(sq.edge_tail)


# ------------------------------------------------------------------------------------------- end to end
@gpu
def test_solve_with_device_assembly_is_the_host_solve_bit_for_bit():
    from gcs_admm_amd import SceneQueries
    As, bs, n, _ = L.region_sets("benchmark4")
    with SceneQueries(As, bs, n) as sq:
        S_, G_ = sq.centers[[0, 37]], sq.centers[[39, 2]]
        host = sq.solve(S_, G_, return_state=True)
        device = sq.solve(S_, G_, return_state=True, assemble="device")
        assert len(host) == len(device) == 2
        for a, b in zip(device, host):
            assert set(a) == set(b)
            assert_same_graphs([a["graph"]], [b["graph"]])
            assert a["trace"].tobytes() == b["trace"].tobytes()
            assert all(a["state"][k].tobytes() == b["state"][k].tobytes() for k in b["state"]) and set(a["state"]) == set(b["state"])
            for k in set(b) - {"graph", "trace", "state", "wall_time_s", "device_time_s"}:
                assert _same_bits(a[k], b[k]), k
            assert np.isfinite(a["rounded_cost"])


def _same_bits(x, y):
    if isinstance(y, dict):
        return isinstance(x, dict) and list(x) == list(y) and all(_same_bits(x[k], y[k]) for k in y)
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
