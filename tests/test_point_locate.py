"""locate_kernel on the host (csrc/point_locate_core.h built by tests/hostemu/locate_emu.cpp: the lanes one after the other, the ballot
from their 64 results) against an extended-precision restatement, and the host assembly of ``gcs_admm_amd.queries.SceneQueries`` on a
stand-in scene against ``graph_from_sets``.  No GPU needed; the same cases go through the kernel in test_gpu_point_locate.py."""
import numpy as np
import pytest

import locate_cases as L
from gcs_admm_amd.graph import convert_pt_to_polytope, graph_from_sets, polytopes_overlap

INT_ARRAYS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr")


def test_chunk_size_is_the_headers():
    """the sizes of locate_cases.py are chosen from it: 600 regions are three chunks with a partial last one"""
    assert L.emu().locate_emu_chunk() == L.CHUNK
    assert -(-600 // L.CHUNK) == 3 and 600 % L.CHUNK != 0 and 600 in L.SIZES


@pytest.mark.parametrize("n", L.DIMS)
@pytest.mark.parametrize("kind,offset", L.FAMILIES)
def test_families_against_the_restatement(kind, offset, n):
    """every P and Q of the family: the list is consistent, sound and complete; UNDECIDED stays a rarity (a kernel that answers
    UNDECIDED everywhere does not pass), and the points do lie in none to several regions"""
    undecided = pairs = 0
    per_point = []
    for P in L.SIZES:
        polys = L.regions(kind, n, P, offset)
        pts = L.points(kind, n, P, offset)
        for Q in L.QUERIES:
            hits = L.family_hits(kind, n, P, offset, Q)
            undecided += L.check_hits(hits, polys, pts[:Q])
            pairs += P * Q
        per_point.append(np.diff(L.family_hits(kind, n, P, offset, max(L.QUERIES))[0]))
    assert undecided <= 1e-3 * pairs, (undecided, pairs)
    assert min(c.min() for c in per_point) == 0 and max(c.max() for c in per_point) >= 2
    assert sum(int((c > 0).sum()) for c in per_point) >= 100


def test_second_call_and_smaller_q_give_the_same_list():
    polys, pts = L.regions("scaled", 3, 600, 300.0), L.points("scaled", 3, 600, 300.0)
    a, b = L.emu_locate(polys, pts), L.emu_locate(polys, pts)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    few = L.emu_locate(polys, pts[:5])
    assert np.array_equal(few[0], a[0][:6]) and np.array_equal(few[1], a[1][:a[0][5]]) and np.array_equal(few[2], a[2][:a[0][5]])


def test_crafted_cases():
    names, polys, pts, expect = L.crafted()
    hits = L.emu_locate(polys, pts)
    L.check_crafted(hits, names, polys, pts, expect)
    # what the LP rule makes of the UNDECIDED ones: on the facet and off the corner the box meets the region ...
    unit = polys[names.index("unit")]
    for q in (0, 1, 3):
        assert polytopes_overlap(*convert_pt_to_polytope(pts[q]), *unit)
    # ... beyond the acute vertex it does not, although every row alone admits a point of the box (rows scaled by 1e3, so that the
    # LP solver's own feasibility tolerance does not decide it)
    A, b = L.WEDGE
    assert not polytopes_overlap(*convert_pt_to_polytope(pts[4]), 1e3 * A, 1e3 * b)
    lo, hi = pts[4] - L.EPS, pts[4] + L.EPS
    for a_i, b_i in zip(A, b):
        assert np.minimum(a_i * lo, a_i * hi).sum() <= b_i


def test_no_points_and_one_region():
    polys = L.regions("boxes", 2, 1)
    hits = L.emu_locate(polys, np.zeros((0, 2)))
    assert L.check_hits(hits, polys, np.zeros((0, 2))) == 0 and len(hits[1]) == 0 and hits[0].tolist() == [0]
    inside = 0.5 * (polys[0][1][:2] - polys[0][1][2:])
    hits = L.emu_locate(polys, np.array([inside, inside + 100.0]))
    assert hits[0].tolist() == [0, 1, 1] and hits[1].tolist() == [0] and hits[2].tolist() == [L.IN]


def test_scan_counts_in_64_bits():
    """the (point, chunk) counts are scanned on the host in 64 bits; a total beyond 2^31 - 1 is refused"""
    lib = L.emu()
    count = np.full(6, 2 ** 30, np.int32)                       # 2 points x 3 chunks
    offset = np.zeros(6, np.int64); hit_ptr = np.zeros(3, np.int64)
    assert lib.locate_emu_scan(count.ctypes.data, 2, 3, offset.ctypes.data, hit_ptr.ctypes.data) == 0
    assert offset.tolist() == [k * 2 ** 30 for k in range(6)] and hit_ptr.tolist() == [0, 3 * 2 ** 30, 6 * 2 ** 30]
    count = np.array([3, 0, 2 ** 31 - 1 - 8, 5, 0, 0], np.int32)              # 3 points x 2 chunks
    hit_ptr = np.zeros(4, np.int64)
    assert lib.locate_emu_scan(count.ctypes.data, 3, 2, offset.ctypes.data, hit_ptr.ctypes.data) == 1
    assert offset.tolist() == [0, 3, 3, 2 ** 31 - 6, 2 ** 31 - 1, 2 ** 31 - 1] and hit_ptr.tolist() == [0, 3, 2 ** 31 - 1, 2 ** 31 - 1]


# ------------------------------------------------------------------------------------------- the host assembly of the query graphs
def make_queries(name, pair_lp=None):
    from gcs_admm_amd.queries import SceneQueries
    As, bs, n, pairs = L.region_sets(name)
    keys = list(As)
    scene = L.EmuScene([(np.asarray(As[k], float), np.asarray(bs[k], float)) for k in keys], pairs)
    return SceneQueries(As, bs, n, scene=scene, pair_lp=pair_lp or L.PairLP()), As, bs, n


def deep_points(sq, count, seed, margin=1e-5):
    """points inside some region and at least ``margin`` (in the row's 1-norm scale) from every facet of every region"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        r = int(rng.integers(len(sq.polys)))
        (A, b), p = sq.polys[r], sq.centers[r] + rng.uniform(-0.3, 0.3, sq.n)
        if all(np.all(np.abs(Ar @ p - br) >= margin * np.abs(Ar).sum(axis=1)) for Ar, br in sq.polys) and np.all(A @ p <= b):
            out.append(p)
    return np.array(out)


def from_scratch(As, bs, n, s, t):
    sets_A = {'s': convert_pt_to_polytope(s)[0], 't': convert_pt_to_polytope(t)[0], **As}
    sets_b = {'s': convert_pt_to_polytope(s)[1], 't': convert_pt_to_polytope(t)[1], **bs}
    return graph_from_sets(sets_A, sets_b, n)


def assert_same_graph(g, ref, s, t):
    assert g.keys == ref.keys and (g.src, g.dst) == (ref.src, ref.dst) == (0, 1) and g.n == ref.n
    for f in INT_ARRAYS:
        a, b = getattr(g, f), getattr(ref, f)
        assert a.dtype == b.dtype and np.array_equal(a, b), f
    assert g.poly_A.tobytes() == ref.poly_A.tobytes() and g.poly_b.tobytes() == ref.poly_b.tobytes()
    assert np.array_equal(g.interior[0], s) and np.array_equal(g.interior[1], t)


@pytest.mark.parametrize("name", ["four_boxes", "benchmark1", "benchmark2", "benchmark3", "benchmark4"])
def test_graphs_equal_graph_from_sets(name):
    lp = L.PairLP()
    sq, As, bs, n = make_queries(name, lp)
    with sq:
        pts = deep_points(sq, 6, seed=len(name))
        S, G = pts[:3], pts[3:]
        graphs = sq.graphs(S, G)
        assert sq.scene.locate_calls == 1 and not lp.calls and sq.last["undecided"] == 0
        for i, g in enumerate(graphs):
            assert_same_graph(g, from_scratch(As, bs, n, S[i], G[i]), S[i], G[i])
            assert np.array_equal(g.interior[2:], sq.centers)
        scene = sq.scene
    assert scene.closed and sq.scene is None


def test_fixture_query_gives_the_committed_graph():
    """benchmark1 with its own start and goal (recovered from its 's' and 't' boxes): the committed edge list, order included"""
    from gcs_admm_amd.cases import fixture_sets, load_fixture
    As_all, bs_all, n, _, _ = fixture_sets("benchmark1")
    case, gref = load_fixture("benchmark1")
    p = lambda k: (np.asarray(bs_all[k])[:n] - np.asarray(bs_all[k])[n:]) / 2
    sq, _, _, _ = make_queries("benchmark1")
    g = sq.graphs([p('s')], [p('t')])[0]
    assert g.keys == case["keys"] and [list(e) for e in g.edges_as_keys()] == case["edges"]
    for f in INT_ARRAYS:
        assert np.array_equal(getattr(g, f), getattr(gref, f)), f


def test_refusals():
    from gcs_admm_amd.queries import SceneQueries
    As, bs, n, pairs = L.region_sets("four_boxes")
    with pytest.raises(ValueError, match="'s' and 't'"):
        SceneQueries({'s': As[0], **As}, {'s': bs[0], **bs}, n, scene=object())
    sq, _, _, _ = make_queries("four_boxes")
    inside, outside = np.array([0.5, 0.5]), np.array([5.0, 5.0])
    with pytest.raises(ValueError, match=r"query 1: the start lies in no region"):
        sq.graphs([inside, outside], [inside, inside])
    with pytest.raises(ValueError, match=r"query 0: the goal lies in no region"):
        sq.graphs([inside], [outside])
    sq.close()
    with pytest.raises(RuntimeError, match="closed"):
        sq.regions_at([inside])


def test_start_and_goal_next_to_each_other():
    sq, As, bs, n = make_queries("four_boxes")
    s = np.array([0.5, 0.5])
    for t, joined in ((s + [1e-6, -1e-6], True), (s + [2.5e-6, 0.0], False)):
        g = sq.graphs([s], [t])[0]
        edges = set(zip(g.edge_tail.tolist(), g.edge_head.tolist()))
        assert ((0, 1) in edges and (1, 0) in edges) == joined and ((0, 1) in edges or (1, 0) in edges) == joined
        assert_same_graph(g, from_scratch(As, bs, n, s, t), s, t)


def test_undecided_hits_go_through_one_lp_call():
    """points on facets and corners of the four boxes: every UNDECIDED hit of the call is in ONE pair LP call, the point box first in
    its pair and its start point p; the graphs are still graph_from_sets'"""
    lp = L.PairLP()
    sq, As, bs, n = make_queries("four_boxes", lp)
    S = np.array([[1.0, 0.5], [0.9, 0.0], [2.0 + 0.5e-6, 0.5]])      # facet of 0 inside 1; corner of 1 on an edge of 0; just off 1, inside 2
    G = np.array([[2.5, 0.5], [3.0, 1.0], [8.5, 8.5]])               # deep in 2; corner of 2; deep in 3
    graphs = sq.graphs(S, G)
    assert sq.scene.locate_calls == 1 and len(lp.calls) == 1
    polys, pa, pb, tol, start = lp.calls[0]
    assert len(pa) == sq.last["undecided"] == 4 and tol == 1e-9
    pts = np.vstack([S, G])
    boxes = len(polys) - len(set(pb.tolist()))
    for a, b in zip(pa, pb):
        p = start[a]
        assert a < boxes <= b and any(np.array_equal(p, q) for q in pts)
        assert all(np.array_equal(x, y) for x, y in zip(polys[a], convert_pt_to_polytope(p)))
        assert any(polys[b][0] is q[0] and polys[b][1] is q[1] for q in sq.polys)
    for i, g in enumerate(graphs):
        assert_same_graph(g, from_scratch(As, bs, n, S[i], G[i]), S[i], G[i])
    assert [r.tolist() for r in sq.regions_at(S)] == [[0, 1], [0, 1], [1, 2]]


def test_failed_lps_are_redone_on_the_host():
    """every pair LP reports status -1 with the wrong flag: the decisions are graph.polytopes_overlap's, the graphs unchanged"""
    sq, As, bs, n = make_queries("four_boxes", L.PairLP(fail=True))
    S, G = np.array([[1.0, 0.5], [2.0 + 0.5e-6, 0.5]]), np.array([[3.0, 1.0], [8.5, 8.5]])
    graphs = sq.graphs(S, G)
    assert sq.last["redone_on_host"] == sq.last["undecided"] >= 3
    for i, g in enumerate(graphs):
        assert_same_graph(g, from_scratch(As, bs, n, S[i], G[i]), S[i], G[i])
