"""The informed region set of a query, the parts that need no GPU: the host build of the path and keep kernels
(tests/hostemu/informed_emu.cpp compiles csrc/informed_core.h, the code the kernels run, the lanes of a round one after the other,
forwards and backwards) against the plain-numpy restatement of informed_cases.py; the refusals; ``SceneQueries.informed`` and
``graphs(prune="informed")`` on a stand-in scene with a host restriction; and seeded errors in a copy of the header, each of which the
checkers must reject.  The kernels themselves: test_gpu_informed.py."""
import numpy as np
import pytest

import informed_cases as I
import locate_cases as L
from gcs_admm_amd import graph as gr
from gcs_admm_amd.queries import SceneQueries
from gcs_admm_amd.scene import edge_arrays
from mutant_build import build_mutants


# ------------------------------------------------------------------------------------------- search
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", I.SCENES)
def test_paths_equal_the_restatement(name, order):
    c = I.case(name)
    e = I.emu_of(c, order)
    assert e.w.tobytes() == I.weights(c.centers, c.tail, c.head).tobytes()      # (the host build contracts nothing at -O1 on x86-64)
    for B in I.BATCHES:
        pts, ptr, reg = c.batch(B)
        got = e.region_paths(pts, ptr, reg)
        ref = I.check_paths(got, c.centers, c.row_ptr, c.tail, c.head, e.w, pts, ptr, reg)
        for i in range(B):      # the settled distances are the restatement's: both are the same fixed point of the same sums
            assert e.last[0][i].tobytes() == ref[i][3].tobytes(), (B, i)


def test_the_cases_hold_what_they_promise():
    got = {}
    for name in I.SCENES:
        c = I.case(name)
        e = I.emu_of(c)
        pts, ptr, reg = c.batch(5)
        got[name] = e.region_paths(pts, ptr, reg) + (e.last[1],)
    assert list(got["islands"][2]) == [1, 1, 0, 0, 0] and np.all(np.isinf(got["islands"][1][:2]))
    assert all(len(p) == 1 for p in got["single"][0])
    assert I.case("boxes300").P > 256 and got["boxes300"][3].max() >= 3      # a lane owns two vertices; several rounds
    assert max(len(p) for p in got["boxes300"][0]) >= 20
    wall, whole = got["lattice_wall"], got["lattice"]
    assert I.case("lattice_wall").P == 43 and wall[1][4] > whole[1][4] + 1.0      # the detour round the wall
    assert I.case("boxes3").n == 3


@pytest.mark.parametrize("name", I.SCENES)
def test_the_order_of_the_lanes_does_not_change_a_bit(name):
    c = I.case(name)
    pts, ptr, reg = c.batch(5)
    runs = []
    for order in (0, 1):
        e = I.emu_of(c, order)
        paths, cost, status = e.region_paths(pts, ptr, reg)
        runs.append((e.last[0].tobytes(), cost.tobytes(), status.tobytes(), [p.tobytes() for p in paths]))
    assert runs[0] == runs[1]


def test_integer_lattice_paths_are_the_restatements_vertex_for_vertex():
    """unit weights and integer points: every sum is exact and most shortest paths tie, so this holds the goal and backtrack tie rules"""
    cen, row_ptr, tail, head, pts, ptr, reg = I.integer_lattice()
    for order in (0, 1):
        e = I.EmuInformed(cen, None, None, row_ptr, tail, head, order)
        assert np.all(e.w == 1.0)
        got = e.region_paths(pts, ptr, reg)
        I.check_paths(got, cen, row_ptr, tail, head, e.w, pts, ptr, reg, exact=True)
        assert list(got[1]) == [14.0, 10.0, 14.0, 0.0, 9.0] and [len(p) for p in got[0]] == [15, 9, 15, 1, 10]
        assert got[0][1][0] == 11 and got[0][1][-1] == 43      # of the two start regions the nearer; of the goal's three equals the smallest


def test_identical_regions_tie_exactly_and_the_smaller_index_wins():
    """lattice_twice: cell r and its copy r + 48 tie in every comparison whatever the centres are -- at the goal (both lie under it), at
    every step back (both explain d) and at the start -- and the rule takes the smaller index each time, without walking the zero-weight
    edge between the two"""
    c = I.case("lattice_twice")
    pts, ptr, reg = c.batch(5)
    assert all(set(r[r >= 48] - 48) == set(r[r < 48]) for r in np.split(reg, ptr[1:-1]))
    for order in (0, 1):
        e = I.emu_of(c, order)
        got = e.region_paths(pts, ptr, reg)
        ref = I.check_paths(got, c.centers, c.row_ptr, c.tail, c.head, e.w, pts, ptr, reg, exact=True)
        assert all(np.array_equal(d[:48], d[48:]) for _, _, _, d in ref)
        assert list(got[2]) == [0] * 5 and all(p.max() < 48 for p in got[0]) and max(len(p) for p in got[0]) >= 10
        whole = I.emu_of(I.case("lattice"), order).region_paths(*I.case("lattice").batch(5))
        assert all(np.array_equal(p, q) for p, q in zip(got[0], whole[0])) and got[1].tobytes() == whole[1].tobytes()


def test_max_len_and_a_cycle_of_identical_centres():
    cen, row_ptr, tail, head, pts, ptr, reg = I.integer_lattice()
    e = I.EmuInformed(cen, None, None, row_ptr, tail, head)
    paths, cost, status = e.region_paths(pts, ptr, reg, max_len=10)
    assert list(status) == [2, 0, 2, 0, 0] and [len(p) for p in paths] == [0, 9, 0, 1, 10] and list(cost) == [14.0, 10.0, 14.0, 0.0, 9.0]
    # regions 0, 1, 2 share one centre and the start lies in region 3 alone: from the goal region 0 the smallest head that explains d
    # is 1, from 1 it is 0, and so on until P steps are taken
    cen = np.array([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
    pa, pb = np.array([2, 0, 1, 0], np.int32), np.array([3, 1, 2, 2], np.int32)
    tail, head = edge_arrays(pa, pb, np.ones(4, np.uint8))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(tail, minlength=4))]).astype(np.int64)
    e = I.EmuInformed(cen, None, None, row_ptr, tail, head)
    pts, ptr, reg = np.array([[0.0, 0.0], [1.0, 0.0]]), np.array([0, 1, 2], np.int64), np.array([3, 0], np.int32)
    paths, cost, status = e.region_paths(pts, ptr, reg)
    assert status[0] == -1 and len(paths[0]) == 0 and cost[0] == 1.0
    assert I.restate_path(cen, row_ptr, head, e.w, pts[0], pts[1], reg[:1], reg[1:])[2] == -1
    paths, cost, status = e.region_paths(pts, ptr, np.array([3, 3], np.int32))      # (start and goal in region 3: nothing to step through)
    assert status[0] == 0 and list(paths[0]) == [3] and cost[0] == 1.0


def test_the_library_bounds_its_workspace():
    chunk = I.emu().inf_emu_chunk
    assert chunk(20000) * 8 * 20000 <= 256 << 20 < (chunk(20000) + 1) * 8 * 20000
    assert chunk(1) == chunk(0) == 65535 and chunk(2 ** 30) == 1


# ------------------------------------------------------------------------------------------- keep
def _bounds(c, e, B):
    """bounds of the first B queries: the centre-polyline cost of each one's candidate path (1.0 where there is none)"""
    pts, ptr, reg = c.batch(B)
    _, cost, status = e.region_paths(pts, ptr, reg)
    return pts, np.where(status == 0, cost, 1.0)


@pytest.mark.parametrize("name", I.SCENES)
def test_flags_equal_the_restatement(name):
    c = I.case(name)
    e = I.emu_of(c)
    for B in I.BATCHES:
        pts, bound = _bounds(c, e, B)
        for scale in (1.0, 1.3, 0.5):
            I.check_keep(e.informed_regions(pts, bound * scale), c.lo, c.hi, pts, bound * scale)
    pts, bound = _bounds(c, e, 5)
    assert e.informed_regions(pts, np.full(5, np.inf)).all()
    for pad in (0.0, 0.25):
        I.check_keep(e.informed_regions(pts, bound, pad), c.lo, c.hi, pts, bound, pad)


def test_a_side_opened_to_infinity_never_counts():
    c = I.case("lattice")
    lo, hi = c.lo.copy(), c.hi.copy()
    lo[7, 0], hi[9, 1], lo[11], hi[11] = -np.inf, np.inf, -np.inf, np.inf
    e = I.EmuInformed(c.centers, lo, hi, c.row_ptr, c.tail, c.head)
    pts, bound = _bounds(c, I.emu_of(c), 5)
    got = e.informed_regions(pts, bound * 0.5)
    I.check_keep(got, lo, hi, pts, bound * 0.5)
    closed = I.emu_of(c).informed_regions(pts, bound * 0.5)
    assert got[:, 11].all() and np.all(got >= closed) and np.any(got != closed)


# ------------------------------------------------------------------------------------------- refused input
def test_refused_input_returns_its_status_and_writes_nothing():
    import re
    c = I.case("boxes2")
    e = I.emu_of(c)
    pts, ptr, reg = c.batch(5)
    cases = I.refusals(c.P, c.n, pts, ptr, reg)
    assert {k for _, _, k, _ in cases} == {"paths", "keep"}
    for label, text, kind, a in cases:
        if kind == "paths":
            outs = [np.full((5, c.P), -3, np.int32), np.full(5, -3, np.int32), np.full(5, -3.0), np.full(5, -3, np.int32)]
            rc = e.raw_paths(a["B"], a["pts"], a["ptr"], a["reg"], a["max_len"], *outs)
        else:
            outs = [np.full((5, c.P), 7, np.uint8)]
            rc = e.raw_keep(a["B"], a["pts"], a["bound"], a["pad"], outs[0])
        assert rc == I.BAD_ARG, label
        assert re.search(text, e.lib.inf_emu_last_error().decode()), (label, e.lib.inf_emu_last_error())
        assert all(np.all(o == (7 if kind == "keep" else -3)) for o in outs), label
    paths, cost, status = e.region_paths(np.zeros((0, 2)), np.zeros(1, np.int64), np.zeros(0, np.int32))      # no query: nothing is done
    assert paths == [] and len(cost) == len(status) == 0
    outs = [np.full((5, c.P), -3, np.int32), np.full(5, -3, np.int32), np.full(5, -3.0), np.full(5, -3, np.int32)]
    assert e.raw_paths(5, pts, np.zeros(11, np.int64), None, c.P, *outs) == I.OK      # queries without a hit, no hit array: no path each
    assert np.all(outs[0] == -1) and np.all(outs[1] == 0) and np.all(np.isinf(outs[2])) and np.all(outs[3] == 1)
    assert e.informed_regions(np.zeros((0, 2)), np.zeros(0)).shape == (0, c.P)


# ------------------------------------------------------------------------------------------- SceneQueries on a stand-in scene
class InformedScene(L.EmuScene):
    """``scene.DeviceScene`` as ``SceneQueries.informed`` uses it, without a device: the two new calls through the host build on the
    stand-in's centres, the exact boxes of its polytopes and the region graph of its pair list as it is when the graph is built"""

    def __init__(self, c):
        up = c.tail < c.head
        L.EmuScene.__init__(self, c.polys, list(zip(c.tail[up].tolist(), c.head[up].tolist())))
        self.case, self.calls, self.graph = c, [], None

    def centers(self):
        return self.case.centers.copy(), np.ones(self.case.P), np.zeros(self.case.P, np.int32)

    def build_region_graph(self, flags=None):
        c = self.case
        self.calls.append("build_region_graph")
        self.graph = I.emu_of(c)
        return len(c.tail)

    def region_paths(self, *a, **k):
        self.calls.append("region_paths")
        return self.graph.region_paths(*a, **k)

    def informed_regions(self, *a, **k):
        self.calls.append("informed_regions")
        return self.graph.informed_regions(*a, **k)


def host_restrict(As, bs, n, paths):
    from gcs_admm_amd.rounding import solve_path_restriction
    return [solve_path_restriction(As, bs, n, p) for p in paths]


@pytest.fixture(scope="module")
def walled():
    """SceneQueries on the walled lattice with its first three queries (two local, one across) and their informed sets, computed once"""
    c = I.case("lattice_wall")
    As = {("cell", r): A for r, (A, _) in enumerate(c.polys)}; bs = {("cell", r): b for r, (_, b) in enumerate(c.polys)}
    calls = []
    def restrict(*a):
        calls.append(a)
        return host_restrict(*a)
    with SceneQueries(As, bs, 2, scene=InformedScene(c), pair_lp=L.PairLP()) as sq:
        S, G = c.S[:3], c.G[:3]
        info = sq.informed(S, G, restrict=restrict)
        yield c, sq, S, G, info, calls


def test_informed_keeps_what_an_optimal_path_can_touch(walled):
    c, sq, S, G, info, calls = walled
    assert sq.scene.calls == ["build_region_graph", "region_paths", "informed_regions"] and len(calls) == 1      # one call each for the batch
    regs = I.regions_under(c.lo, c.hi, np.vstack([S, G]))
    paths, cost, _ = I.emu_of(c).region_paths(*c.batch(3))
    for i, rec in enumerate(info):
        assert set(rec) == {"path", "bound", "keep", "restriction"}
        assert np.array_equal(rec["path"], paths[i]) and rec["keep"].dtype == bool and rec["keep"].shape == (c.P,)
        # the bound is a feasible path's length: finite, and at least the straight line between the two boxes
        assert np.linalg.norm(S[i] - G[i]) - 4e-6 <= rec["bound"] < np.inf
        assert list(rec["restriction"]) == ['s'] + [("cell", int(r)) for r in rec["path"]] + ['t']
        inside = np.array([I.dist(S[i], m) + I.dist(m, G[i]) <= rec["bound"] for m in c.centers])
        assert inside.any() and np.all(rec["keep"][inside])
        assert np.all(rec["keep"][regs[i]]) and np.all(rec["keep"][regs[3 + i]]) and np.all(rec["keep"][rec["path"]])
        want, _ = I.restate_keep(c.lo, c.hi, S[i], G[i], rec["bound"] + 4 * I.EPS * np.sqrt(2))
        want[regs[i]] = want[regs[3 + i]] = True
        assert np.array_equal(rec["keep"], want)
    assert info[0]["keep"].sum() < c.P and info[1]["keep"].sum() < c.P      # the local queries lose regions


def test_an_infeasible_or_failed_restriction_keeps_every_region(walled):
    c, sq, S, G, _, _ = walled
    for result in ((float("inf"), None), (float("inf"), {"s": np.zeros(4)}), (float("nan"), {"s": np.zeros(4)})):
        info = sq.informed(S[:2], G[:2], restrict=lambda As, bs, n, paths: [result] * len(paths))
        assert all(np.isinf(r["bound"]) and r["keep"].all() and r["restriction"] is None and len(r["path"]) > 0 for r in info)
    isl = I.case("islands")
    As = {r: A for r, (A, _) in enumerate(isl.polys)}; bs = {r: b for r, (_, b) in enumerate(isl.polys)}
    with SceneQueries(As, bs, 2, scene=InformedScene(isl), pair_lp=L.PairLP()) as other:
        info = other.informed(isl.S[:1], isl.G[:1], restrict=lambda *a: pytest.fail("no path: nothing to restrict"))
        assert len(info[0]["path"]) == 0 and np.isinf(info[0]["bound"]) and info[0]["keep"].all()


FIELDS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr", "poly_A", "poly_b", "interior")


def pruned_reference(sq, s, g, rs, rt, keep, eps=1e-6):
    """``graph._finish_graph`` on the edge list of the induced subgraph, masked and renumbered here"""
    idx = np.nonzero(keep)[0]
    new = np.full(len(keep), -1, np.int64)
    new[idx] = np.arange(len(idx))
    both = keep[sq.edge_tail] & keep[sq.edge_head]
    edges = [(int(new[u]) + 2, int(new[v]) + 2) for u, v in zip(sq.edge_tail[both], sq.edge_head[both])]
    edges += [(0, int(new[r]) + 2) for r in rs] + [(int(new[r]) + 2, 0) for r in rs] + [(1, int(new[r]) + 2) for r in rt] + [(int(new[r]) + 2, 1) for r in rt]
    if np.all(np.abs(s - g) <= 2 * eps + 1e-9):
        edges += [(0, 1), (1, 0)]
    edges.sort()
    polys = [gr.convert_pt_to_polytope(s, eps), gr.convert_pt_to_polytope(g, eps)] + [sq.polys[r] for r in idx]
    return gr._finish_graph(sq.n, ['s', 't'] + [sq.keys[r] for r in idx], np.array([e[0] for e in edges], np.int64), np.array([e[1] for e in edges], np.int64),
                            polys, np.vstack([s, g, sq.centers[idx]]), 0, 1)


def assert_same_graph(g, h):
    assert (g.n, g.keys, g.src, g.dst) == (h.n, h.keys, h.src, h.dst) and type(g.keys) is list
    for f in FIELDS:
        a, b = getattr(g, f), getattr(h, f)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f


def test_pruned_graphs_are_the_host_path_on_the_induced_subgraph(walled):
    c, sq, S, G, info, _ = walled
    got = sq.graphs(S, G, prune="informed", restrict=host_restrict)
    regs = I.regions_under(c.lo, c.hi, np.vstack([S, G]))
    for i, g in enumerate(got):
        assert g.num_vertices == 2 + int(info[i]["keep"].sum())
        assert_same_graph(g, pruned_reference(sq, S[i], G[i], regs[i], regs[3 + i], info[i]["keep"]))
    whole = sq.graphs(S, G)
    for g, h in zip(sq.graphs(S, G, prune=None), whole):
        assert_same_graph(g, h)
    full = np.ones(c.P, bool)
    for i, h in enumerate(whole):      # nothing pruned: the graph of the whole scene, through the same assembly
        assert_same_graph(h, pruned_reference(sq, S[i], G[i], regs[i], regs[3 + i], full))
        assert_same_graph(h, sq._host_graph(S[i], G[i], regs[i], regs[3 + i], 1e-6, full))
    assert got[0].num_vertices < whole[0].num_vertices


def test_a_solved_candidate_joins_the_rounding_candidates():
    """``rounding_many(extra=...)``, the way ``solve(prune=...)`` hands in the bound's path: the cheapest of the walks' candidates and
    the extra ones wins, in the shape of every other result"""
    from gcs_admm_amd.rounding import rounding_many
    V = ['s', 'a', 'b', 't']
    E = [('s', 'a'), ('a', 't'), ('s', 'b'), ('b', 't')]
    out = {'s': [E[0], E[2]], 'a': [E[1]], 'b': [E[3]], 't': []}
    x = {v: np.full(4, float(i)) for i, v in enumerate(V)}
    problem = dict(y_e_sol={E[0]: 1.0, E[1]: 1.0, E[2]: 0.0, E[3]: 0.0}, V=V, E=E, I_v_out=out, As={v: None for v in V}, bs={v: None for v in V}, n=2)
    solver = lambda As, bs, n, paths: [(5.0, {k: x[k[1]] for k in p}) for p in paths]      # every walk (s, a, t) costs 5
    via_b = {k: x[k] for k in ('s', 'b', 't')}
    assert rounding_many([problem], solver=solver)[0][0] == 5.0
    cost, x_v, y_v = rounding_many([problem], solver=solver, extra=[[(4.0, ['s', 'b', 't'], via_b)]])[0]
    assert cost == 4.0 and y_v == {'s': 1, 'a': 0, 'b': 1, 't': 1} and np.array_equal(x_v['b'], x['b']) and np.array_equal(x_v['a'], np.zeros(4))
    cost, _, y_v = rounding_many([problem], solver=solver, extra=[[(6.0, ['s', 'b', 't'], via_b)]])[0]
    assert cost == 5.0 and y_v == {'s': 1, 'a': 1, 'b': 0, 't': 1}
    assert rounding_many([problem], solver=solver, extra=[[]])[0][0] == 5.0


def test_prune_is_refused_with_device_assembly_and_by_any_other_name(walled):
    _, sq, S, G, _, _ = walled
    before = list(sq.scene.calls)
    for call in (sq.graphs, sq.solve):
        with pytest.raises(ValueError, match="prune needs assemble='host'"):
            call(S, G, prune="informed", assemble="device")
        with pytest.raises(ValueError, match="prune must be None or 'informed'"):
            call(S, G, prune="ellipse")
    assert sq.scene.calls == before


# ------------------------------------------------------------------------------------------- seeded errors
# (anchor in informed_core.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "largest_goal_among_equals": [("if (c < best) { best = c; goal = r; }", "if (c <= best) { best = c; goal = r; }")],
    "init_of_every_region": [("return at < q.a && q.rs[at] == v ? informed_distance(", "return at <= q.a ? informed_distance(")],
    "relax_skips_the_last_entry": [("for (long long p = g.row_ptr[v]; p < last; ++p) best = fmin(", "for (long long p = g.row_ptr[v]; p < last - 1; ++p) best = fmin(")],
    "pad_moves_the_sides_in": [("fmax(fmax(lo[k] - pad - p[k], 0.0), p[k] - hi[k] - pad)", "fmax(fmax(lo[k] + pad - p[k], 0.0), p[k] - hi[k] + pad)")],
    "one_distance": [("return informed_box_distance(s, lo, hi, n, pad) + informed_box_distance(g, lo, hi, n, pad);", "return informed_box_distance(s, lo, hi, n, pad);")],
}
SEEDED = [m for m in MUTANTS if m != "clean"]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    return {name: I.declare(lib) for name, lib in build_mutants(tmp_path_factory.mktemp("informed_mutants"), "informed_core.h", MUTANTS, I.EMU_SRC).items()}


def _violations(lib):
    missed = []
    c = I.case("boxes2")
    e = I.emu_of(c, lib=lib)
    pts, ptr, reg = c.batch(5)
    try:
        I.check_paths(e.region_paths(pts, ptr, reg), c.centers, c.row_ptr, c.tail, c.head, I.weights(c.centers, c.tail, c.head), pts, ptr, reg)
        cen, row_ptr, tail, head, ipts, iptr, ireg = I.integer_lattice()
        x = I.EmuInformed(cen, None, None, row_ptr, tail, head, lib=lib)
        I.check_paths(x.region_paths(ipts, iptr, ireg), cen, row_ptr, tail, head, x.w, ipts, iptr, ireg, exact=True)
    except AssertionError:
        missed.append("paths")
    try:
        bound = np.array([3.0, 2.0, 8.0, 5.0, 6.0])
        I.check_keep(e.informed_regions(pts, bound, 0.25), c.lo, c.hi, pts, bound, 0.25)
    except AssertionError:
        missed.append("keep")
    return missed


def test_clean_copy_passes(builds):
    assert _violations(builds["clean"]) == []


@pytest.mark.parametrize("mutant", SEEDED)
def test_seeded_errors_are_rejected(builds, mutant):
    assert _violations(builds[mutant]) == [["paths"], ["keep"]][mutant in ("pad_moves_the_sides_in", "one_distance")], mutant
