"""The device assembly of pruned query graphs (csrc/induced_graph_core.h) through its host build, without a device: the induced graphs
of every scene, batch and keep pattern of induced_graph_cases.py against the host path's masked and renumbered edge list, with the
lanes run forwards and backwards and in every chunking; the sizes; the refusals; seeded errors in a copy of the header; and
``SceneQueries.graphs(prune="informed", assemble="induced")`` on a stand-in scene against the host-pruned graphs.  The kernels run the
same tables in test_gpu_induced_graph.py."""
import numpy as np
import pytest

import induced_graph_cases as G
import informed_cases as I
import locate_cases as L
import query_graph_cases as Q
from gcs_admm_amd import SceneQueries
from mutant_build import build_mutants

# ------------------------------------------------------------------------------------------- the graphs
@pytest.mark.parametrize("name", G.SCENES)
def test_induced_graphs_equal_the_host_path(name):
    seen = 0
    with G.emu_of(name) as fwd, G.emu_of(name, backwards=True) as bwd:
        for pattern in G.PATTERNS:
            for B in G.batches_of(name, pattern):
                made = G.batch(name, B, pattern)
                if made is None:
                    continue
                keep, ptr, reg, st = made
                label = (name, pattern, B)
                ref = G.reference(name, keep, ptr, reg, st)
                want_kept, want_edges = G.reference_sizes(ref)
                assert np.array_equal(want_kept, (keep != 0).sum(axis=1)), label
                num_kept, num_edges = fwd.induced_sizes(keep, ptr, reg, st)
                assert num_kept.dtype == np.int32 and num_edges.dtype == np.int64
                assert np.array_equal(num_kept, want_kept) and np.array_equal(num_edges, want_edges), label
                runs = [fwd.induced_query_graphs(keep, ptr, reg, st, chunk) for chunk in G.CHUNKS]
                G.assert_same(runs[0], ref, label)
                assert G.same_bytes(runs[0], runs[1]) and G.same_bytes(runs[0], runs[2]), label
                assert G.same_bytes(runs[0], bwd.induced_query_graphs(keep, ptr, reg, st, 3)), label
                seen += 1
    assert seen >= 2 * (len(G.PATTERNS) - 3)


@pytest.mark.parametrize("name", G.SCENES)
def test_all_kept_is_the_assembly_of_the_whole_scene(name):
    """nothing pruned: byte for byte what the query-graph code that is already in use writes"""
    P, pa, pb = G.scene_pairs(name)
    with Q.EmuGraph(P, pa, pb, np.ones(len(pa), np.uint8)) as whole, G.emu_of(name) as e:
        whole.build_region_graph()
        for mine, theirs in zip(G.region_graph(name)[1:], whole.region_graph()):
            assert mine.dtype == theirs.dtype and mine.tobytes() == theirs.tobytes()
        for B in (1, 5):
            keep, ptr, reg, st = G.batch(name, B, "all")
            assert G.same_bytes(e.induced_query_graphs(keep, ptr, reg, st), whole.query_graphs(ptr, reg, st))


def test_the_patterns_are_what_they_say():
    P, row_ptr, tail, head, _ = G.region_graph("boxes600")
    for count in (64, 65, 256, 257):
        keep, ptr, reg, st = G.batch("boxes600", 5, "first%d" % count)
        assert np.all((keep != 0).sum(axis=1) == count) and np.all(keep[:, :count] != 0) and reg.max() < count
    keep, ptr, reg, st = G.batch("boxes130", 5, "lone_hit")
    r = int(reg[0])
    P, row_ptr, tail, head, _ = G.region_graph("boxes130")
    assert row_ptr[r + 1] > row_ptr[r] and not keep[:, head[row_ptr[r]:row_ptr[r + 1]]].any()      # a hit of induced degree 0
    keep, ptr, reg, st = G.batch("hub", 5, "hub_dropped")
    assert not keep[:, 0].any() and reg.min() >= 1
    keep, ptr, reg, st = G.batch("hub", 5, "hub_and_three_leaves")
    assert np.all((keep != 0).sum(axis=1) == 4) and keep[:, 0].all()
    assert G.batch("boxes65", 2, "hub_dropped") is None and G.batch("apart", 2, "lone_hit") is None
    assert len(G.region_graph(G.LATTICE)[2]) == 2 * (24 * 40 + 25 * 39 + 2 * 24 * 39)


def test_no_query_and_no_region_graph():
    with G.emu_of("boxes65") as e:
        assert e.induced_query_graphs(np.zeros((0, 65), np.uint8), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8)) == []
        assert e.raw_sizes(0, None, None, None, None, None, None) == G.OK and e.raw_graphs(0, *[None] * 4, 0, *[None] * 9) == G.OK
        keep, ptr, reg, st = G.batch("boxes65", 2, "random0.5")
        before = e.induced_query_graphs(keep, ptr, reg, st)
        e.invalidate()                                                      # what an edit does to the graph
        for call in (lambda: e.induced_sizes(keep, ptr, reg, st), lambda: e.induced_query_graphs(keep, ptr, reg, st)):
            with pytest.raises(Q.EmuError, match=r"region graph.*status 1"):
                call()
    with G.emu_of("boxes65") as e:
        assert G.same_bytes(before, e.induced_query_graphs(keep, ptr, reg, st))
    assert G.emu().ige_chunk(20000, 79202, 0) >= 1 and G.emu().ige_chunk(20000, 79202, 7) == 7 and G.emu().ige_chunk(1, 0, 10 ** 6) == 65535
    assert G.emu().ige_chunk(2 * 10 ** 6, 3 * 10 ** 7, 0) == 1                  # one query is above the bound: one per launch


# ------------------------------------------------------------------------------------------- refusals
def test_refused_input_returns_its_status_and_writes_nothing():
    with G.emu_of("boxes130") as e:
        G.check_refusals(e.raw_sizes, e.raw_graphs, e.error)


# ------------------------------------------------------------------------------------------- SceneQueries on a stand-in scene
class InducedScene(L.EmuScene):
    """``scene.DeviceScene`` as ``SceneQueries`` uses it with ``prune="informed"``, without a device: the informed calls and the induced
    assembly through their host builds, on the stand-in's centres, the exact boxes of its polytopes and the region graph of its pair
    list"""

    def __init__(self, c):
        up = c.tail < c.head
        L.EmuScene.__init__(self, c.polys, list(zip(c.tail[up].tolist(), c.head[up].tolist())))
        self.case, self.calls, self.informed, self.induced = c, [], None, None

    def centers(self):
        return self.case.centers.copy(), np.ones(self.case.P), np.zeros(self.case.P, np.int32)

    def build_region_graph(self, flags=None):
        c = self.case
        self.calls.append("build_region_graph")
        self.informed, self.induced = I.emu_of(c), G.EmuInduced(c.P, c.row_ptr, c.tail, c.head, G.reverse_edges(c.tail, c.head))
        return len(c.tail)

    def region_paths(self, *a, **k):
        self.calls.append("region_paths")
        return self.informed.region_paths(*a, **k)

    def informed_regions(self, *a, **k):
        self.calls.append("informed_regions")
        return self.informed.informed_regions(*a, **k)

    def induced_query_graphs(self, *a, **k):
        self.calls.append("induced_query_graphs")
        return self.induced.induced_query_graphs(*a, **k)


def host_restrict(As, bs, n, paths):
    from gcs_admm_amd.rounding import solve_path_restriction
    return [solve_path_restriction(As, bs, n, p) for p in paths]


@pytest.fixture(scope="module")
def walled():
    c = I.case("lattice_wall")
    As = {("cell", r): A for r, (A, _) in enumerate(c.polys)}; bs = {("cell", r): b for r, (_, b) in enumerate(c.polys)}
    with SceneQueries(As, bs, 2, scene=InducedScene(c), pair_lp=L.PairLP()) as sq:
        yield c, sq, c.S[:5], c.G[:5]


def test_scene_queries_induced_assembly_equals_the_host_pruned_graphs(walled):
    c, sq, S, G_ = walled
    host, info = sq._graphs(S, G_, 1e-6, 1e-9, "host", "informed", host_restrict)
    sq.scene.calls.clear()
    got = sq.graphs(S, G_, prune="informed", assemble="induced", restrict=host_restrict)
    assert sq.scene.calls == ["region_paths", "informed_regions", "induced_query_graphs"]      # one call for the batch
    regs = I.regions_under(c.lo, c.hi, np.vstack([S, G_]))
    assert len(got) == len(host) == 5
    for i, (g, h) in enumerate(zip(got, host)):
        G.assert_same_graph(g, h)
        G.assert_same_graph(g, sq._host_graph(S[i], G_[i], regs[i], regs[5 + i], 1e-6, info[i]["keep"]))
        assert g.num_vertices == 2 + int(info[i]["keep"].sum())
    assert got[0].num_vertices < 2 + c.P                                     # a local query loses regions
    assert sq.graphs(np.zeros((0, 2)), np.zeros((0, 2)), prune="informed", assemble="induced") == []


def test_induced_needs_prune_and_the_other_refusals_stay(walled):
    _, sq, S, G_ = walled
    before = list(sq.scene.calls)
    for call in (sq.graphs, sq.solve):
        with pytest.raises(ValueError, match=r"^assemble='induced' needs prune$"):
            call(S, G_, assemble="induced")
        with pytest.raises(ValueError, match="prune needs assemble='host'"):
            call(S, G_, prune="informed", assemble="device")
        with pytest.raises(ValueError, match="assemble must be 'host' or 'device'"):
            call(S, G_, prune="informed", assemble="gpu")
    assert sq.scene.calls == before


# ------------------------------------------------------------------------------------------- seeded errors
# (anchor in induced_graph_core.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "tile_carry_dropped": [("sum += tile_total;", "sum += 0 * tile_total;")],
    "tile_carry_not_applied": [("return sum + within;", "return within;")],
    "head_flag_not_tested": [("d += q.keep[g.head[p]] ? 1 : 0;", "d += 1;")],
    "reverse_from_the_unpruned_offset": [("(int)(q.row_ptr[jw] + q.rank[", "(int)(g.row_ptr[w] + q.rank[")],
    "goal_list_not_renumbered": [("term_new[g_at] = newidx[b.term_region[g_at]];", "term_new[g_at] = b.term_region[g_at];")],
}
SEEDED = [m for m in MUTANTS if m != "clean"]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    return {name: G.declare(lib) for name, lib in build_mutants(tmp_path_factory.mktemp("induced_mutants"), "induced_graph_core.h", MUTANTS, G.EMU_SRC).items()}


def _violations(lib):
    """what a build gets wrong on the tile carry's lattice and on 130 boxes: the sizes first, and the graphs only where the sizes hold
    (the arrays are laid out by them)"""
    missed = []
    for name, pattern in ((G.LATTICE, "random0.5"), ("boxes130", "random0.5"), ("boxes130", "lone_hit")):
        keep, ptr, reg, st = G.batch(name, 5, pattern)
        ref = G.reference(name, keep, ptr, reg, st)
        with G.emu_of(name, lib=lib) as e:
            num_kept, num_edges = e.induced_sizes(keep, ptr, reg, st)
            want = G.reference_sizes(ref)
            if not (np.array_equal(num_kept, want[0]) and np.array_equal(num_edges, want[1])):
                missed.append((name, pattern, "sizes"))
                continue
            try:
                G.assert_same(e.induced_query_graphs(keep, ptr, reg, st), ref)
            except (AssertionError, Q.EmuError):
                missed.append((name, pattern, "graphs"))
    return missed


def test_clean_copy_passes(builds):
    assert _violations(builds["clean"]) == []


@pytest.mark.parametrize("mutant", SEEDED)
def test_seeded_errors_are_rejected(builds, mutant):
    assert _violations(builds[mutant]), mutant
