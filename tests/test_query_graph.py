"""The device assembly of query graphs, the parts that need no GPU: the host build of the region-graph and query-graph kernels
(tests/hostemu/query_graph_emu.cpp compiles csrc/query_graph_core.h, the code the kernels run, with the threads one after the other, the
library's checks and its chunks) against ``scene.edge_arrays`` and against the host path of ``SceneQueries.graphs`` +
``graph._finish_graph``, element for element; the refusals; ``SceneQueries.graphs(assemble="device")`` on stand-in scenes against
``assemble="host"`` field by field; and seeded errors in a copy of the header, each of which the checkers must reject.  The kernels
themselves: test_gpu_query_graph.py."""
import ctypes as C

import numpy as np
import pytest

import locate_cases as L
import query_graph_cases as Q
from gcs_admm_amd import graph as gr
from gcs_admm_amd.queries import SceneQueries
from mutant_build import build_mutants
from test_scene_edit import FakeEditScene


@pytest.fixture(scope="module")
def emu():
    return Q.emu()


# ------------------------------------------------------------------------------------------- region graph
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("name", Q.SCENES)
def test_region_graph_equals_edge_arrays(emu, name, shuffled):
    P, pa, pb = Q.scene_pairs(name, shuffled)
    if name == "identical":
        assert len(pa) == 330 * 329 // 2
    if name == "apart":
        assert len(pa) == 0
    for density in Q.DENSITIES:
        flags = Q.random_flags(len(pa), density)
        with Q.EmuGraph(P, pa, pb, flags) as g:
            assert g.build_region_graph() == 2 * int((flags != 0).sum())
            got = g.region_graph()
            Q.check_region_graph(got, P, pa, pb, flags)
            if name == "hub" and density == 1.0:
                assert np.diff(got[0])[0] == 599 and np.all(np.diff(got[0])[1:] == 1)


def test_region_graph_does_not_depend_on_the_order_of_the_pairs(emu):
    P, pa, pb = Q.scene_pairs("boxes600")
    flags = Q.random_flags(len(pa), 0.5)
    with Q.EmuGraph(P, pa, pb, flags) as g:
        g.build_region_graph()
        first = g.region_graph()
    o = np.random.default_rng(5).permutation(len(pa))
    with Q.EmuGraph(P, pa[o], pb[o], flags[o]) as g:
        g.build_region_graph()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, g.region_graph()))


def test_host_flags_take_the_place_of_the_resident_ones(emu):
    P, pa, pb = Q.scene_pairs("boxes130")
    resident, host = Q.random_flags(len(pa), 0.5), Q.random_flags(len(pa), 0.5, seed=1)
    assert np.any((resident != 0) != (host != 0))
    with Q.EmuGraph(P, pa, pb, resident) as g:
        g.build_region_graph(host)
        Q.check_region_graph(g.region_graph(), P, pa, pb, host)
        g.build_region_graph()                                     # the resident flags are as they were
        Q.check_region_graph(g.region_graph(), P, pa, pb, resident)


def test_too_many_edges_are_refused_by_the_scan(emu):
    """2 (E_R + 4 P + 2) <= 2^31 - 1 is what keeps every query graph's incidence indices in 32 bits"""
    P = 70000
    row_ptr = np.empty(P + 1, np.int64)
    count = np.full(P, 69999, np.int32)
    assert emu.qg_emu_scan(count.ctypes.data, P, row_ptr.ctypes.data) == 0 and row_ptr[-1] == P * 69999
    count[:] = 15000                                               # 1.05e9 edges: 2 E = 2.1e9 and a little, just inside
    assert emu.qg_emu_scan(count.ctypes.data, P, row_ptr.ctypes.data) == 1
    assert np.array_equal(row_ptr, np.arange(P + 1, dtype=np.int64) * 15000)
    count[:] = 15340                                               # 2 (1 073 800 000 + 280 002) > 2^31 - 1
    assert emu.qg_emu_scan(count.ctypes.data, P, row_ptr.ctypes.data) == 0
    assert emu.qg_emu_scan(None, 0, row_ptr.ctypes.data) == 1 and row_ptr[0] == 0


# ------------------------------------------------------------------------------------------- query graphs
def _built(name, density, seed=0):
    P, pa, pb = Q.scene_pairs(name)
    flags = Q.random_flags(len(pa), density, seed)
    g = Q.EmuGraph(P, pa, pb, flags)
    g.build_region_graph()
    return g


@pytest.mark.parametrize("density", Q.DENSITIES)
@pytest.mark.parametrize("P", Q.REGIONS)
def test_query_graphs_equal_the_host_path(emu, P, density):
    with _built("boxes%d" % P, density) as g:
        row_ptr, tail, head, _ = g.region_graph()
        for B in Q.BATCHES:
            term_ptr, term_region, st = Q.hit_lists(P, B, np.diff(row_ptr), seed=B)
            runs = [g.query_graphs(term_ptr, term_region, st, chunk) for chunk in Q.CHUNKS]
            Q.check_query_graphs(runs[0], tail, head, P, term_ptr, term_region, st)
            assert Q.same_bytes(runs[0], runs[1]) and Q.same_bytes(runs[0], runs[2])


def test_hit_lists_hold_what_the_cases_promise():
    P = 130
    with _built("boxes130", 0.1) as g:
        degree = np.diff(g.region_graph()[0])
    assert np.any(degree == 0)
    term_ptr, reg, st = Q.hit_lists(P, 5, degree)
    lists = np.split(reg, term_ptr[1:-1])
    assert {len(l) for l in lists} >= {1, 2} and max(len(l) for l in lists) >= 10
    assert set(lists[0]) <= set(lists[5]) and np.array_equal(lists[1], lists[6]) and st[1] == 1
    assert lists[2][0] == 0 and lists[7][-1] == P - 1
    assert degree[lists[8][0]] == 0 and any(degree[r] == 0 for r in lists[3])
    assert all(np.all(np.diff(l) > 0) for l in lists)


@pytest.mark.parametrize("name", ["identical", "hub", "apart"])
def test_query_graphs_on_the_extreme_degrees(emu, name):
    with _built(name, 1.0) as g:
        row_ptr, tail, head, _ = g.region_graph()
        term_ptr, term_region, st = Q.hit_lists(g.P, 5, np.diff(row_ptr))
        for chunk in (0, 3):
            Q.check_query_graphs(g.query_graphs(term_ptr, term_region, st, chunk), tail, head, g.P, term_ptr, term_region, st)


def test_an_empty_hit_list_is_a_vertex_without_edges(emu):
    with _built("boxes65", 1.0) as g:
        _, tail, head, _ = g.region_graph()
        term_ptr = np.array([0, 0, 2, 2, 3], np.int64)             # query 0: no start hit; query 1: no goal hit... and one with both
        term_region = np.array([3, 9, 64], np.int32)
        st = np.array([1, 0], np.uint8)
        got = g.query_graphs(term_ptr, term_region, st)
        Q.check_query_graphs(got, tail, head, g.P, term_ptr, term_region, st)
        assert got[0][2][1] == 2 and got[1][2][2] - got[1][2][1] == 2        # inc_ptr: s has the s-t pair alone; t one hit
        none = g.query_graphs(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8))
        assert none == []


def test_the_library_bounds_its_workspace(emu):
    P, E_R = 20000, 400000
    chunk = emu.qg_emu_chunk(P, E_R, 0)
    per_query = 4 * (8 * (E_R + 4 * P + 2) + P + 3)
    assert chunk >= 1 and chunk * per_query <= 256 << 20 < (chunk + 1) * per_query
    assert emu.qg_emu_chunk(P, 10 ** 9, 0) == 1                    # one query is more than the bound: one at a time
    assert emu.qg_emu_chunk(1, 0, 0) == 65535 and emu.qg_emu_chunk(P, E_R, 7) == 7 and emu.qg_emu_chunk(P, E_R, 10 ** 6) == 65535


# ------------------------------------------------------------------------------------------- refused input
def _raw(g, a, outs):
    ptr = lambda x: None if x is None else x.ctypes.data
    return g.lib.qg_emu_query(g.h, a["B"], ptr(a["ptr"]), ptr(a["reg"]), ptr(a["st"]), a["chunk"], ptr(a["off"]), *(o.ctypes.data for o in outs))


def test_refused_input_returns_its_status_and_changes_nothing(emu):
    import re
    with _built("boxes130", 1.0) as g:
        P, E_R = g.P, g.num_region_edges
        graph = g.region_graph()
        term_ptr, term_region, st = Q.hit_lists(P, 5, np.diff(graph[0]), seed=1)
        off = Q.edge_offsets(E_R, term_ptr, st)
        cases = Q.refusals(P, E_R, term_ptr, term_region, st)
        assert len(cases) >= 12 and {status for _, status, _, _ in cases} == {Q.BAD_ARG, Q.UNSUPPORTED}
        for label, status, text, a in cases:
            outs = Q.raw_outputs(5, P, int(off[-1]))
            assert _raw(g, a, outs) == status, label
            assert re.search(text, g.lib.qg_emu_last_error(g.h).decode()), (label, g.lib.qg_emu_last_error(g.h))
            assert all(np.all(o == -3) for o in outs), label
            assert all(x.tobytes() == y.tobytes() for x, y in zip(graph, g.region_graph())), label
        outs = Q.raw_outputs(5, P, int(off[-1]))                   # the valid call the refusals were made from
        ok = dict(B=5, ptr=term_ptr, reg=term_region, st=st, chunk=0, off=off)
        assert _raw(g, ok, outs) == Q.OK and not any(np.any(o == -3) for o in outs)
        # a stale graph (an edit, a new narrow phase) and no graph at all
        g.invalidate()
        outs = Q.raw_outputs(5, P, int(off[-1]))
        assert _raw(g, ok, outs) == Q.BAD_ARG and "region graph" in g.lib.qg_emu_last_error(g.h).decode()
        assert all(np.all(o == -3) for o in outs)
        with pytest.raises(Q.EmuError, match="region graph"):
            g.region_graph()
        g.build_region_graph()
        assert _raw(g, ok, outs) == Q.OK


# ------------------------------------------------------------------------------------------- SceneQueries on stand-in scenes
class _Assembly:
    """the three new methods of ``scene.DeviceScene`` for a stand-in scene, through the host build: the region graph is built from the
    stand-in's pair list and flags as they are when ``build_region_graph`` is called, and ends with every edit"""
    emu_graph = None

    def build_region_graph(self, flags=None):
        pa, pb, resident, _ = self.pairs()
        if self.emu_graph is not None:
            self.emu_graph.close()
        self.emu_graph = Q.EmuGraph(len(self.polys), pa, pb, resident)
        self.assembly_calls.append(("build_region_graph", None if flags is None else np.array(flags)))
        return self.emu_graph.build_region_graph(flags)

    def region_graph(self):
        return self.emu_graph.region_graph()

    def query_graphs(self, term_ptr, term_region, st_adjacent, chunk_queries=0):
        self.assembly_calls.append(("query_graphs", len(st_adjacent)))
        return self.emu_graph.query_graphs(term_ptr, term_region, st_adjacent, chunk_queries)

    def _edited(self):
        if self.emu_graph is not None:
            self.emu_graph.invalidate()


class AssemblyScene(_Assembly, L.EmuScene):
    def __init__(self, polys, pairs):
        L.EmuScene.__init__(self, polys, pairs)
        self.assembly_calls = []


class AssemblyEditScene(_Assembly, FakeEditScene):
    def __init__(self, polys, **fake):
        FakeEditScene.__init__(self, polys, **fake)
        self.assembly_calls = []

    def add_regions(self, *a, **k):
        self._edited()
        return FakeEditScene.add_regions(self, *a, **k)

    def remove_regions(self, *a, **k):
        self._edited()
        return FakeEditScene.remove_regions(self, *a, **k)


FIELDS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr", "poly_A", "poly_b", "interior")


def assert_same_graphs(got, ref):
    assert len(got) == len(ref) > 0
    for g, h in zip(got, ref):
        assert (g.n, g.keys, g.src, g.dst) == (h.n, h.keys, h.src, h.dst) and type(g.keys) is list
        for f in FIELDS:
            a, b = getattr(g, f), getattr(h, f)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f
            assert a.flags["C_CONTIGUOUS"], f


def _points(sq, count, seed=0):
    rng = np.random.default_rng(seed + len(sq.keys))
    return sq.centers[rng.integers(0, len(sq.keys), count)]


@pytest.mark.parametrize("name", ["four_boxes", "benchmark1", "benchmark2", "benchmark3", "benchmark4"])
def test_scene_queries_device_assembly_equals_the_host_path(name):
    As, bs, n, pairs = L.region_sets(name)
    scene = AssemblyScene([(np.asarray(As[k], float), np.asarray(bs[k], float).ravel()) for k in As], pairs)
    with SceneQueries(As, bs, n, scene=scene, pair_lp=L.PairLP()) as sq:
        B = 5
        pts = _points(sq, 2 * B)
        if name == "four_boxes":
            pts[0], pts[B] = (0.95, 0.5), (0.95, 0.5)                          # start = goal in two regions: rs == rt, c = 1
        ref = sq.graphs(pts[:B], pts[B:])
        assert scene.assembly_calls == []                                      # the default path calls none of the new methods
        got = sq.graphs(pts[:B], pts[B:], assemble="device")
        assert_same_graphs(got, ref)
        assert_same_graphs(sq.graphs(pts[:2], pts[B:B + 2], assemble="device"), ref[:2])
        assert [c[0] for c in scene.assembly_calls] == ["build_region_graph", "query_graphs", "query_graphs"]      # built once, one call a batch
        assert scene.assembly_calls[0][1] is None                              # no undecided pair: the resident flags
        assert scene.assembly_calls[1][1] == B


def test_scene_queries_device_assembly_with_undecided_hits():
    names, polys, pts, _ = L.crafted(zero_rows=False)
    As = {k: A for k, (A, _) in zip(names, polys)}; bs = {k: b for k, (_, b) in zip(names, polys)}
    pairs = [(i, j) for i in range(len(polys)) for j in range(i + 1, len(polys)) if gr.polytopes_overlap(*polys[i], *polys[j])]
    lp = L.PairLP()
    with SceneQueries(As, bs, 2, scene=AssemblyScene(polys, pairs), pair_lp=lp) as sq:
        got = sq.graphs(pts[:4], pts[4:], assemble="device")
        assert sq.last["undecided"] > 0 and len(lp.calls) == 1
        assert_same_graphs(got, sq.graphs(pts[:4], pts[4:]))


def _edit_queries(As, bs, n, keys, **fake):
    A = {k: As[k] for k in keys}; b = {k: bs[k] for k in keys}
    return SceneQueries(A, b, n, scene=AssemblyEditScene([(A[k], b[k]) for k in keys], **fake), pair_lp=L.PairLP())


def _edit_regions():
    As, bs, n, _ = L.region_sets("benchmark4")
    return {k: np.asarray(As[k], float) for k in As}, {k: np.asarray(bs[k], float).ravel() for k in bs}, n


def test_a_pair_decided_on_the_host_is_in_the_device_graph():
    from test_scene_edit import _sig
    from gcs_admm_amd import scene as sc
    As, bs, n = _edit_regions()
    keys = list(As)
    polys = [(As[k], bs[k]) for k in keys]
    pa, pb = sc.candidate_pairs(*FakeEditScene(polys)._boxes())
    over = [t for t in range(len(pa)) if gr.polytopes_overlap(*polys[pa[t]], *polys[pb[t]])][:2]
    apart = [t for t in range(len(pa)) if not gr.polytopes_overlap(*polys[pa[t]], *polys[pb[t]])][:1]
    assert len(over) == 2 and len(apart) == 1
    undecided = [(_sig(polys[pa[t]]), _sig(polys[pb[t]])) for t in over + apart]      # status -1 and the WRONG flag on the scene
    with _edit_queries(As, bs, n, keys, undecided=undecided) as sq, _edit_queries(As, bs, n, keys) as clean:
        assert sq.stats["overlaps_redone_on_host"] == 3
        assert np.array_equal(sq.edge_tail, clean.edge_tail)                   # the host's decisions are the right ones
        pts = _points(sq, 4)
        got = sq.graphs(pts[:2], pts[2:], assemble="device")
        assert_same_graphs(got, sq.graphs(pts[:2], pts[2:]))
        assert_same_graphs(got, clean.graphs(pts[:2], pts[2:], assemble="device"))
        call = sq.scene.assembly_calls[0]
        assert call[0] == "build_region_graph" and np.array_equal(call[1], sq._pairs["flags"])
        assert not np.array_equal(sq.scene.pairs()[2], sq._pairs["flags"])     # the scene's own flags would have given another graph
        assert clean.scene.assembly_calls[0][1] is None


def test_device_assembly_follows_add_and_remove():
    As, bs, n = _edit_regions()
    keys = list(As)
    part = lambda ks: ({k: As[k] for k in ks}, {k: bs[k] for k in ks})
    with _edit_queries(As, bs, n, keys[:-6]) as sq:
        pts = _points(sq, 6)
        assert_same_graphs(sq.graphs(pts[:3], pts[3:], assemble="device"), sq.graphs(pts[:3], pts[3:]))
        stacked = sq._stacked
        sq.add_regions(*part(keys[-6:]))
        assert sq._stacked is not stacked and len(sq._stacked[0]) == len(keys) + 1
        pts = _points(sq, 6, seed=1)
        pts[0] = sq.centers[-1]                                                # a start in an added region
        got = sq.graphs(pts[:3], pts[3:], assemble="device")
        assert_same_graphs(got, sq.graphs(pts[:3], pts[3:]))
        with _edit_queries(As, bs, n, keys) as whole:
            assert_same_graphs(got, whole.graphs(pts[:3], pts[3:], assemble="device"))
        sq.remove_regions([keys[1], keys[-2], keys[5]])
        assert len(sq._stacked[0]) == len(keys) - 2 and sq._stacked[1].shape[0] == sq._stacked[0][-1] == len(sq._stacked[2])
        pts = _points(sq, 6, seed=2)
        assert_same_graphs(sq.graphs(pts[:3], pts[3:], assemble="device"), sq.graphs(pts[:3], pts[3:]))
        builds = [c for c in sq.scene.assembly_calls if c[0] == "build_region_graph"]
        assert len(builds) == 3                                                # once, and again after each edit
    with _edit_queries(As, bs, n, keys[:-6]) as sq:                            # edits before the first device call: nothing to follow
        sq.add_regions(*part(keys[-6:])); sq.remove_regions([keys[0]])
        assert sq._stacked is None and sq.scene.assembly_calls == []
        pts = _points(sq, 4)
        assert_same_graphs(sq.graphs(pts[:2], pts[2:], assemble="device"), sq.graphs(pts[:2], pts[2:]))


def test_the_errors_of_graphs_are_those_of_the_host_path():
    As, bs, n, pairs = L.region_sets("four_boxes")
    scene = AssemblyScene([(np.asarray(As[k], float), np.asarray(bs[k], float).ravel()) for k in As], pairs)
    with SceneQueries(As, bs, n, scene=scene, pair_lp=L.PairLP()) as sq:
        inside, outside = np.array([[0.5, 0.5]]), np.array([[5.0, 5.0]])
        for assemble in ("host", "device"):
            with pytest.raises(ValueError, match="query 0: the start lies in no region"):
                sq.graphs(outside, inside, assemble=assemble)
            with pytest.raises(ValueError, match="query 0: the goal lies in no region"):
                sq.graphs(inside, outside, assemble=assemble)
            with pytest.raises(ValueError, match="one goal for every start"):
                sq.graphs(np.vstack([inside, inside]), inside, assemble=assemble)
        for bad in ("gpu", "", None):
            with pytest.raises(ValueError, match="assemble must be 'host' or 'device'"):
                sq.graphs(inside, inside, assemble=bad)
            with pytest.raises(ValueError, match="assemble must be 'host' or 'device'"):
                sq.solve(inside, inside, assemble=bad)
        assert scene.assembly_calls == []


# ------------------------------------------------------------------------------------------- seeded errors
# (anchor in query_graph_core.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "le_for_lt": [("return g.row_ptr[r] + query_terminal_edges(k) + x.lt;", "return g.row_ptr[r] + query_terminal_edges(k) + x.le;")],
    "dropped_in_rs": [("query_put_edge(o, down + x.in_s, r + 2, 1,", "query_put_edge(o, down, r + 2, 1,")],
    "halves_swapped": [("const long long in_slot = base + h + k, out_slot = base + 2 * h + d + k;",
                        "const long long out_slot = base + h + k, in_slot = base + 2 * h + d + k;")],
    "rev_from_the_wrong_row": [("graph_lower_bound(g.head, g.row_ptr[w], g.row_ptr[w + 1], u)", "graph_lower_bound(g.head, g.row_ptr[u], g.row_ptr[u + 1], u)")],
}
SEEDED = [m for m in MUTANTS if m != "clean"]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    return {name: Q.declare(lib) for name, lib in build_mutants(tmp_path_factory.mktemp("query_graph_mutants"), "query_graph_core.h", MUTANTS, Q.EMU_SRC).items()}


def _violations(lib):
    """the checks of this file that a build misses, on one scene: the region graph, and the query graphs of five queries"""
    P, pa, pb = Q.scene_pairs("boxes65")
    flags = Q.random_flags(len(pa), 1.0)
    missed = []
    with Q.EmuGraph(P, pa, pb, flags, lib=lib) as g:
        g.build_region_graph()
        row_ptr, tail, head, rev = g.region_graph()
        try:
            Q.check_region_graph((row_ptr, tail, head, rev), P, pa, pb, flags)
        except AssertionError:
            missed.append("region graph")
        term_ptr, term_region, st = Q.hit_lists(P, 5, np.diff(row_ptr))
        # (a wrong reverse edge is an index into the region graph, so every index stays inside the chunk's buffers)
        try:
            Q.check_query_graphs(g.query_graphs(term_ptr, term_region, st), tail, head, P, term_ptr, term_region, st)
        except AssertionError:
            missed.append("query graphs")
    return missed


def test_clean_copy_passes(builds):
    assert _violations(builds["clean"]) == []


@pytest.mark.parametrize("mutant", SEEDED)
def test_seeded_errors_are_rejected(builds, mutant):
    missed = _violations(builds[mutant])
    assert "query graphs" in missed, mutant
    assert ("region graph" in missed) == (mutant == "rev_from_the_wrong_row")
