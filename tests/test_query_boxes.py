"""``SceneQueries`` with start and goal BOXES (``start_boxes`` / ``goal_boxes``, ``regions_meeting``) on the stand-in scenes of
test_query_graph.py, against ``graph.graph_from_sets`` on ``{'s': box, 't': box, regions}``: every field of every graph by dtype, shape
and bytes, in both ``assemble`` modes, for box / box, point / box and box / point queries, for terminals that overlap each other, and
the refusals.  The stand-in's ``locate_boxes`` is the host build of locate_box_kernel (locate_box_cases.py).  No GPU."""
import numpy as np
import pytest

import locate_box_cases as bxc
import locate_cases as L
from gcs_admm_amd.graph import convert_pt_to_polytope, graph_from_sets
from gcs_admm_amd.queries import SceneQueries
from test_query_graph import FIELDS, AssemblyScene, assert_same_graphs


class BoxScene(AssemblyScene):
    """AssemblyScene with the one call the box queries add"""

    def __init__(self, polys, pairs):
        AssemblyScene.__init__(self, polys, pairs)
        self.box_calls = 0

    def locate_boxes(self, lo, hi, tol=L.TOL):
        self.box_calls += 1
        return bxc.emu_locate_boxes(self.polys, lo, hi, tol, n=self.n)


def queries_on(name):
    As, bs, n, pairs = L.region_sets(name)
    scene = BoxScene([(np.asarray(As[k], float), np.asarray(bs[k], float).ravel()) for k in As], pairs)
    return As, bs, n, scene, SceneQueries(As, bs, n, scene=scene, pair_lp=L.PairLP())


def terminals(sq, B, seed=0):
    """B start boxes, goal boxes and points on the scene of ``sq``: boxes around region centres, half-widths from 0.02 to 0.6 of the
    scene's extent per region (a thin box inside one region up to a box across several), and points at other centres"""
    rng = np.random.default_rng(seed + len(sq.keys))
    P = len(sq.keys)
    pick = lambda: sq.centers[rng.integers(0, P, B)]
    cs, cg = pick() + rng.uniform(-0.05, 0.05, (B, sq.n)), pick() + rng.uniform(-0.05, 0.05, (B, sq.n))
    hs, hg = 10.0 ** rng.uniform(-2, 0, (B, sq.n)), 10.0 ** rng.uniform(-2, 0, (B, sq.n))
    return (cs - hs, cs + hs), (cg - hg, cg + hg), pick(), pick()


def reference(As, bs, n, s, t):
    """graph_from_sets on {'s', 't', regions}; a terminal is (lo, hi) or a point"""
    poly = lambda x: (np.vstack([np.eye(n), -np.eye(n)]), np.hstack([x[1], -x[0]])) if isinstance(x, tuple) else convert_pt_to_polytope(x)
    sets_A, sets_b = {'s': poly(s)[0], 't': poly(t)[0], **As}, {'s': poly(s)[1], 't': poly(t)[1], **bs}
    return graph_from_sets(sets_A, sets_b, n)


def assert_graph_is_reference(g, ref, s, t, centers):
    """field for field; for a terminal that is a point the interior is the point itself (graph_from_sets has the centre of its box,
    which may differ from it in the last place), as for every point query"""
    assert (g.n, g.keys, g.src, g.dst) == (ref.n, ref.keys, ref.src, ref.dst)
    for f in FIELDS:
        a, b = getattr(g, f), getattr(ref, f)
        assert a.dtype == b.dtype and a.shape == b.shape, f
        if f != "interior":
            assert a.tobytes() == b.tobytes(), f
    for v, term in enumerate((s, t)):
        if isinstance(term, tuple):
            assert g.interior[v].tobytes() == ref.interior[v].tobytes() == (0.5 * (term[0] + term[1])).tobytes()
        else:
            assert g.interior[v].tobytes() == np.asarray(term, float).tobytes() and np.allclose(g.interior[v], ref.interior[v], rtol=0, atol=1e-12)
    assert g.interior[2:].tobytes() == ref.interior[2:].tobytes() == centers.tobytes()


@pytest.mark.parametrize("assemble", ["host", "device"])
@pytest.mark.parametrize("name", ["four_boxes", "benchmark1", "benchmark3"])
def test_graphs_with_box_terminals_equal_graph_from_sets(name, assemble):
    As, bs, n, scene, sq = queries_on(name)
    B = 3
    with sq:
        sb, gb, ps, pg = terminals(sq, B)
        row = lambda boxes, i: (boxes[0][i], boxes[1][i])
        # box / box: one locate_boxes call for all starts and goals, no locate call
        graphs = sq.graphs(start_boxes=sb, goal_boxes=gb, assemble=assemble)
        assert (scene.box_calls, scene.locate_calls) == (1, 0) and sq.last["hits"] > 0
        for i, g in enumerate(graphs):
            assert_graph_is_reference(g, reference(As, bs, n, row(sb, i), row(gb, i)), row(sb, i), row(gb, i), sq.centers)
        # point / box, the common case, and box / point: one call of each kind
        graphs = sq.graphs(starts=ps, goal_boxes=gb, assemble=assemble)
        assert (scene.box_calls, scene.locate_calls) == (2, 1)
        for i, g in enumerate(graphs):
            assert_graph_is_reference(g, reference(As, bs, n, ps[i], row(gb, i)), ps[i], row(gb, i), sq.centers)
        graphs = sq.graphs(goals=pg, start_boxes=sb, assemble=assemble)
        for i, g in enumerate(graphs):
            assert_graph_is_reference(g, reference(As, bs, n, row(sb, i), pg[i]), row(sb, i), pg[i], sq.centers)
        # the point queries are what they were
        assert_same_graphs(sq.graphs(ps, pg, assemble=assemble), sq.graphs(starts=ps, goals=pg))


@pytest.mark.parametrize("assemble", ["host", "device"])
def test_terminals_that_overlap_each_other_are_joined(assemble):
    """s and t overlap (an s-t edge both ways), touch in a vertex (joined: touching counts), and lie 1e-6 apart (not joined); a point
    start inside the goal box is joined to it"""
    As, bs, n, scene, sq = queries_on("four_boxes")
    lo_s = np.array([[0.1, 0.1], [0.1, 0.1], [0.1, 0.1]]); hi_s = np.array([[0.6, 0.6], [0.5, 0.5], [0.5, 0.5]])
    lo_t = np.array([[0.4, 0.4], [0.5, 0.5], [0.5 + 1e-6, 0.1]]); hi_t = np.array([[0.9, 0.9], [0.9, 0.9], [0.9, 0.9]])
    with sq:
        graphs = sq.graphs(start_boxes=(lo_s, hi_s), goal_boxes=(lo_t, hi_t), assemble=assemble)
        joined = [(0, 1) in set(zip(g.edge_tail.tolist(), g.edge_head.tolist())) for g in graphs]
        assert joined == [True, True, False]
        for i, g in enumerate(graphs):
            s, t = (lo_s[i], hi_s[i]), (lo_t[i], hi_t[i])
            assert_graph_is_reference(g, reference(As, bs, n, s, t), s, t, sq.centers)
        p = np.array([[0.5, 0.5]])
        g = sq.graphs(starts=p, goal_boxes=(lo_t[:1], hi_t[:1]), assemble=assemble)[0]
        assert (0, 1) in set(zip(g.edge_tail.tolist(), g.edge_head.tolist()))
        assert_graph_is_reference(g, reference(As, bs, n, p[0], (lo_t[0], hi_t[0])), p[0], (lo_t[0], hi_t[0]), sq.centers)


def test_regions_meeting_decides_its_undecided_hits_in_one_lp_call():
    """a box across three of the four boxes: the regions that do not hold its centre are UNDECIDED and go, all boxes together, through
    one pair-LP call -- the box first in every pair, started at its centre; a failed LP is decided by polytopes_overlap"""
    for fail in (False, True):
        As, bs, n, pairs = L.region_sets("four_boxes")
        polys = [(np.asarray(As[k], float), np.asarray(bs[k], float)) for k in As]
        lp = L.PairLP(fail=fail)
        lo = np.array([[0.5, 0.2], [8.2, 8.2], [4.0, 4.0]]); hi = np.array([[2.5, 0.8], [8.4, 8.4], [5.0, 5.0]])
        with SceneQueries(As, bs, n, scene=BoxScene(polys, pairs), pair_lp=lp) as sq:
            regs = sq.regions_meeting(lo, hi)
            assert [r.tolist() for r in regs] == [[0, 1, 2], [3], []] and all(r.dtype == np.int32 for r in regs)
            assert len(lp.calls) == 1
            lp_polys, pa, pb, tol, start = lp.calls[0]
            assert sq.last == dict(hits=4, undecided=2, redone_on_host=2 if fail else 0)
            assert pa.tolist() == [0, 0] and [lp_polys[i][1].tolist() for i in pb] == [polys[0][1].tolist(), polys[2][1].tolist()]
            assert lp_polys[0][0].tolist() == np.vstack([np.eye(2), -np.eye(2)]).tolist() and lp_polys[0][1].tolist() == [2.5, 0.8, -0.5, -0.2]
            assert start[0].tolist() == [1.5, 0.5] and tol == 1e-9


def test_refusals():
    As, bs, n, scene, sq = queries_on("four_boxes")
    box = (np.array([[0.2, 0.2]]), np.array([[0.6, 0.6]]))
    p = np.array([[0.5, 0.5]])
    with sq:
        for kw in (dict(starts=p, start_boxes=box, goals=p), dict(goals=p), dict(starts=p), dict(starts=p, goals=p, goal_boxes=box), dict()):
            with pytest.raises(ValueError, match="exactly one of"):
                sq.graphs(**kw)
        with pytest.raises(ValueError, match="prune='informed' takes point terminals"):
            sq.graphs(starts=p, goal_boxes=box, prune="informed")
        with pytest.raises(ValueError, match="prune='informed' takes point terminals"):
            sq.graphs(start_boxes=box, goal_boxes=box, prune="informed", assemble="induced")
        for thin in ((np.array([[0.2, 0.2]]), np.array([[0.6, 0.2 + 2e-5]])), (np.array([[0.2, 0.2]]), np.array([[0.2, 0.2]])),
                     (np.array([[0.6, 0.2]]), np.array([[0.2, 0.6]]))):
            with pytest.raises(ValueError, match="every half-width must exceed 1e-05"):
                sq.graphs(starts=p, goal_boxes=thin)
            with pytest.raises(ValueError, match="every half-width must exceed 1e-05"):
                sq.graphs(start_boxes=thin, goals=p)
        with pytest.raises(ValueError, match="one goal for every start"):
            sq.graphs(starts=np.vstack([p, p]), goal_boxes=box)
        with pytest.raises(ValueError, match="query 0: the goal lies in no region"):
            sq.graphs(starts=p, goal_boxes=(np.array([[4.0, 4.0]]), np.array([[5.0, 5.0]])))
        # nothing of this reached the scene but the one located query
        assert scene.box_calls == 1
