"""The device assembly of pruned query graphs on the device (gcsadmm_scene_induced_sizes / _induced_query_graphs in csrc/polytope_lp.hip
through scene.DeviceScene and queries.SceneQueries): the graphs of every scene, batch and keep pattern of induced_graph_cases.py against
the host path's masked and renumbered edge list and against the host build of the same code, in every chunking; the refusals; the
lifecycle across edits; ``SceneQueries.graphs`` and ``solve`` with ``prune="informed", assemble="induced"`` against the host-pruned
ones, bit for bit.  The host build runs the same tables without a device in test_induced_graph.py."""
import numpy as np
import pytest

import induced_graph_cases as G
import locate_cases as L
import query_graph_cases as Q
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError

gpu = pytest.mark.gpu

NEW_KERNELS = ("induced_count_kernel", "induced_build_kernel", "induced_graph_kernel")


def test_new_kernels_use_no_scratch():
    """(no device needed: the compiler's resource remarks of the in-tree build)"""
    from gcs_admm_amd import build
    res = build.kernel_resources()
    for name in NEW_KERNELS:
        mine = {k: v for k, v in res.items() if name in k}
        assert len(mine) == 1, (name, sorted(mine))
        assert all(v["scratch"] == 0 for v in mine.values()), mine


def decided(name):
    """a scene of boxes (the caller closes it) whose resident region graph is ``induced_graph_cases.region_graph(name)``: the exact
    boxes set by hand, the sweep at pad 0, and every pair of it an edge"""
    lo, hi = G.scene_boxes(name)
    scene = sc.DeviceScene(Q.box_polys(lo, hi))
    try:
        scene.centers(); scene.set_boxes(lo, hi); scene.candidate_pairs(0.0); scene.overlaps(1e-9)
        scene.build_region_graph(np.ones(scene.num_pairs, np.uint8))
        for mine, theirs in zip(G.region_graph(name)[1:], scene.region_graph()):
            assert mine.dtype == theirs.dtype and mine.tobytes() == theirs.tobytes()
    except Exception:
        scene.close()
        raise
    return scene


# ------------------------------------------------------------------------------------------- the graphs
@gpu
@pytest.mark.parametrize("name", G.SCENES)
def test_induced_graphs_equal_the_host_path_and_the_host_build(name):
    with decided(name) as scene, G.emu_of(name) as emu:
        for pattern in G.PATTERNS:
            for B in G.batches_of(name, pattern):
                made = G.batch(name, B, pattern)
                if made is None:
                    continue
                keep, ptr, reg, st = made
                label = (name, pattern, B)
                ref = G.reference(name, keep, ptr, reg, st)
                num_kept, num_edges = scene.induced_sizes(keep, ptr, reg, st)
                want = G.reference_sizes(ref)
                assert np.array_equal(num_kept, want[0]) and np.array_equal(num_edges, want[1]), label
                runs = [scene.induced_query_graphs(keep, ptr, reg, st, chunk) for chunk in G.CHUNKS]
                G.assert_same(runs[0], ref, label)
                assert G.same_bytes(runs[0], runs[1]) and G.same_bytes(runs[0], runs[2]), label
                assert G.same_bytes(runs[0], emu.induced_query_graphs(keep, ptr, reg, st)), label
        keep, ptr, reg, st = G.batch(name, 5, "all")                        # nothing pruned: the assembly of the whole scene
        assert G.same_bytes(scene.induced_query_graphs(keep, ptr, reg, st), scene.query_graphs(ptr, reg, st))
        assert scene.induced_query_graphs(np.zeros((0, scene.P), np.uint8), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8)) == []


# ------------------------------------------------------------------------------------------- refusals, lifecycle
@gpu
def test_refused_input_returns_its_status_and_changes_nothing():
    with decided("boxes130") as scene:
        graph = scene.region_graph()
        G.check_refusals(lambda *a: scene.lib.gcsadmm_scene_induced_sizes(scene._h, *a), lambda *a: scene.lib.gcsadmm_scene_induced_query_graphs(scene._h, *a),
                       lambda: scene.lib.gcsadmm_polytope_last_error().decode())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(graph, scene.region_graph()))
    with sc.DeviceScene(Q.box_polys(*Q.scene_boxes("boxes65"))) as scene:       # no region graph yet
        scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps(1e-9)
        keep, ptr, reg, st = G.batch("boxes65", 2, "random0.5")
        with pytest.raises(GcsAdmmError, match=r"no resident region graph.*status 1"):
            scene.induced_query_graphs(keep, ptr, reg, st)


@gpu
def test_an_edit_ends_the_graph_and_a_rebuild_follows_it():
    lo, hi = Q.scene_boxes("boxes130")
    polys = Q.box_polys(lo, hi)
    with sc.DeviceScene(polys[:100]) as scene:
        scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps(1e-9)
        scene.build_region_graph()

        def batch():
            P = scene.P
            rng = np.random.default_rng(P)
            _, tail, head, _ = scene.region_graph()
            ptr, reg, st = Q.hit_lists(P, 5, np.bincount(tail, minlength=P), seed=2)
            keep = G._force_hits((rng.random((5, P)) < 0.5).astype(np.uint8), ptr, reg)
            return tail, head, keep, ptr, reg, st

        tail, head, keep, ptr, reg, st = batch()
        G.assert_same(scene.induced_query_graphs(keep, ptr, reg, st), G.reference_on(tail, head, keep, ptr, reg, st))
        for edit in (lambda: scene.add_regions(polys[100:]), lambda: scene.remove_regions([0, 50, 129])):
            edit()
            P = scene.P
            stale = (np.ones((1, P), np.uint8), np.array([0, 1, 2], np.int64), np.array([3, 7], np.int32), np.array([0], np.uint8))
            for call in (lambda: scene.induced_query_graphs(*stale), lambda: scene.induced_sizes(*stale)):
                with pytest.raises(GcsAdmmError, match=r"region graph.*status 1"):
                    call()
            scene.build_region_graph()
            tail, head, keep, ptr, reg, st = batch()
            G.assert_same(scene.induced_query_graphs(keep, ptr, reg, st), G.reference_on(tail, head, keep, ptr, reg, st))
        assert scene.P == 127


# ------------------------------------------------------------------------------------------- SceneQueries against its host-pruned path
def assert_same_graphs(got, ref):
    assert len(got) == len(ref) > 0
    for g, h in zip(got, ref):
        G.assert_same_graph(g, h)


def _points(sq, count, seed=0):
    rng = np.random.default_rng(seed + len(sq.keys))
    return sq.centers[rng.integers(0, len(sq.keys), count)]


@gpu
@pytest.mark.parametrize("name", ["benchmark1", "benchmark2", "benchmark3", "benchmark4"])
def test_scene_queries_induced_assembly_equals_the_host_pruned_path(name):
    from gcs_admm_amd import SceneQueries
    As, bs, n, _ = L.region_sets(name)
    with SceneQueries(As, bs, n) as sq:
        pts = _points(sq, 10)
        pts[5] = pts[0]                                             # start = goal
        assert_same_graphs(sq.graphs(pts[:5], pts[5:], prune="informed", assemble="induced"), sq.graphs(pts[:5], pts[5:], prune="informed"))


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
            pts = _points(sq, 8, seed)
            pts[4] = sq.centers[(np.argmin(np.abs(sq.centers - pts[0]).sum(axis=1)) + 1) % len(sq.keys)]      # one local query
            got = sq.graphs(pts[:4], pts[4:], prune="informed", assemble="induced")
            assert_same_graphs(got, sq.graphs(pts[:4], pts[4:], prune="informed"))
            return got
        assert min(g.num_vertices for g in both(0)) < 972
        sq.add_regions(*part(keys[-30:]))
        assert max(g.num_vertices for g in both(1)) <= 1002
        sq.remove_regions(keys[3:400:7])
        assert max(g.num_vertices for g in both(2)) <= 1002 - len(keys[3:400:7])
        assert sq.scene.num_region_edges == len(sq.edge_tail)


# ------------------------------------------------------------------------------------------- end to end
def _same_bits(x, y):
    if isinstance(y, dict):
        return isinstance(x, dict) and list(x) == list(y) and all(_same_bits(x[k], y[k]) for k in y)
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@gpu
@pytest.mark.parametrize("walk", ["host", "device"])
def test_pruned_solve_with_induced_assembly_is_the_host_pruned_solve_bit_for_bit(walk):
    from gcs_admm_amd import SceneQueries
    As, bs, n, _ = L.region_sets("benchmark4")
    with SceneQueries(As, bs, n) as sq:
        S_, G_ = sq.centers[[0, 37]], sq.centers[[39, 2]]
        host = sq.solve(S_, G_, return_state=True, prune="informed", walk=walk)
        induced = sq.solve(S_, G_, return_state=True, prune="informed", assemble="induced", walk=walk)
        assert len(host) == len(induced) == 2
        for a, b in zip(induced, host):
            assert set(a) == set(b)
            G.assert_same_graph(a["graph"], b["graph"])
            assert a["trace"].tobytes() == b["trace"].tobytes()
            assert all(a["state"][k].tobytes() == b["state"][k].tobytes() for k in b["state"]) and set(a["state"]) == set(b["state"])
            for k in set(b) - {"graph", "trace", "state", "wall_time_s", "device_time_s"}:
                assert _same_bits(a[k], b[k]), k
            assert np.isfinite(a["rounded_cost"])
