"""The informed region set between start and goal SETS, the parts that need no GPU: the host build of the set kernels
(tests/hostemu/informed_set_emu.cpp compiles csrc/informed_set_core.h, the code the kernels run, the lanes of a round one after the other,
forwards and backwards, under the newest bound or the one of the round before) against the kernels for points on degenerate boxes, bit
for bit, and against the plain-numpy restatement of informed_set_cases.py, which runs its search to the end; the soundness of the box
distance; the refusals; ``SceneQueries.informed_sets`` and ``graphs(prune="informed_sets")`` on a stand-in scene with a host
restriction; and seeded errors in a copy of the header.  The kernels themselves: test_gpu_informed_sets.py."""
import re

import numpy as np
import pytest

import induced_graph_cases as G
import informed_cases as I
import informed_set_cases as T
import locate_box_cases as bxc
import locate_cases as L
from gcs_admm_amd.queries import SceneQueries
from mutant_build import build_mutants
from test_informed import InformedScene, assert_same_graph, host_restrict


# ------------------------------------------------------------------------------------------- degenerate boxes: the point kernels' bits
@pytest.mark.parametrize("name", I.SCENES)
def test_degenerate_boxes_give_the_bits_of_the_point_calls(name):
    c = I.case(name)
    point = I.emu_of(c)
    for order in T.ORDERS:
        sets = T.emu_of(c, order)
        assert sets.w.tobytes() == point.w.tobytes()
        for B in I.BATCHES:
            pts, ptr, reg = c.batch(B)
            want = point.region_paths(pts, ptr, reg)
            got = sets.region_paths_sets(pts, pts, ptr, reg)
            assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes(), (order, B)
            assert all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(got[0], want[0])), (order, B)
            bound = np.where(want[2] == 0, want[1], 1.0)
            for scale, pad in ((1.0, T.SWEEP_PAD), (1.3, 0.0), (0.5, 0.25)):
                assert np.array_equal(sets.informed_regions_sets(pts, pts, bound * scale, pad), point.informed_regions(pts, bound * scale, pad))
    outs = [[np.full((5, 7), -1, np.int32), np.zeros(5, np.int32), np.zeros(5), np.zeros(5, np.int32)] for _ in range(2)]
    pts, ptr, reg = c.batch(5)      # max_len below the paths' lengths: the raw arrays of both
    assert point.raw_paths(5, pts, ptr, reg, 7, *outs[0]) == T.emu_of(c).raw_paths(5, pts, pts, ptr, reg, 7, *outs[1]) == I.OK
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))


# ------------------------------------------------------------------------------------------- boxes: the search run to the end
@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("name", I.SCENES)
def test_box_terminals_equal_the_restatement(name, kind):
    c = I.case(name)
    for half in T.HALF_WIDTHS:
        tlo, thi, ptr, reg = T.batch(c, 5, kind, half)
        runs = []
        for order in T.ORDERS:
            e = T.emu_of(c, order)
            got = e.region_paths_sets(tlo, thi, ptr, reg)
            ref = T.check_paths(got, c.centers, c.row_ptr, c.tail, c.head, e.w, tlo, thi, ptr, reg, exact=name == "lattice_twice")
            d, rounds = e.last
            for i in range(5):
                T.check_distances(d[i], ref[i])
                if ref[i][2] == 0:      # the costs bit for bit: both are the same sums
                    assert got[1][i] == ref[i][1], (half, order, i)
            assert np.all(rounds >= 1) and np.all(rounds <= c.P)
            runs.append((got[1].tobytes(), got[2].tobytes(), [p.tobytes() for p in got[0]]))
        assert all(r == runs[0] for r in runs[1:])      # the order of the lanes and a lagging bound change no result
        e = T.emu_of(c)
        # (1.0 where there is no path, and where the two boxes share a centre: at a bound of 0 every region on both boxes is at the threshold)
        bound = np.array([r[1] if r[2] == 0 and r[1] > 0 else 1.0 for r in ref])
        for scale in (1.0, 1.3, 0.5):
            T.check_keep(e.informed_regions_sets(tlo, thi, bound * scale), c.lo, c.hi, tlo, thi, bound * scale)
        for pad in (0.0, 0.25):
            T.check_keep(e.informed_regions_sets(tlo, thi, bound, pad), c.lo, c.hi, tlo, thi, bound, pad)


def test_the_bound_ends_a_local_search_early():
    """what the bound is for: on boxes300 the two local queries settle in fewer rounds than the search that runs to the end, with most
    distances never written; the query across the scene cannot gain"""
    c = I.case("boxes300")
    pts, ptr, reg = c.batch(3)
    point, sets = I.emu_of(c), T.emu_of(c)
    point.region_paths(pts, ptr, reg); sets.region_paths_sets(pts, pts, ptr, reg)
    (d_all, r_all), (d, r) = point.last, sets.last
    assert np.all(r <= r_all) and np.all(r[:2] < r_all[:2])
    assert np.all(np.isfinite(d).sum(axis=1)[:2] < 0.5 * np.isfinite(d_all).sum(axis=1)[:2])


def test_a_terminal_that_meets_more_regions_than_there_are_lanes():
    c = I.case("boxes300")
    tlo, thi, ptr, reg = T.wide_batch(c)
    for order in T.ORDERS:
        e = T.emu_of(c, order)
        got = e.region_paths_sets(tlo, thi, ptr, reg)
        ref = T.check_paths(got, c.centers, c.row_ptr, c.tail, c.head, e.w, tlo, thi, ptr, reg)
        for i in range(2):
            T.check_distances(e.last[0][i], ref[i])
        assert list(got[2]) == [0, 0] and len(got[0][0]) == 1 and got[0][0][0] in reg[ptr[0]:ptr[1]]      # the goal box holds the start's region
        bound = np.maximum(got[1], 0.5)
        T.check_keep(e.informed_regions_sets(tlo, thi, bound), c.lo, c.hi, tlo, thi, bound)


# ------------------------------------------------------------------------------------------- the two distances
def test_the_gap_of_two_boxes_is_exact_and_below_every_pair_of_points():
    lib = T.emu()
    rng = np.random.default_rng(5)
    a = lambda x: x.ctypes.data
    for trial in range(200):
        n = int(rng.integers(1, 5))
        ca, cb = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
        ha, hb = rng.uniform(0, 1.5, n) * (rng.random(n) < 0.8), rng.uniform(0.05, 1.5, n)
        tlo, thi, lo, hi = ca - ha, ca + ha, cb - hb, cb + hb
        pad = [0.0, 0.1][trial % 2]
        got = lib.inf_set_emu_gap(n, a(tlo), a(thi), a(lo), a(hi), pad)
        per_axis = np.maximum(np.maximum((lo - pad) - thi, 0.0), tlo - (hi + pad))      # the distance of two intervals
        assert abs(got - np.sqrt(np.sum(per_axis ** 2))) <= 4 * np.finfo(float).eps * got
        assert got == T.gap(tlo, thi, lo[None], hi[None], pad)[0]
        p = tlo + rng.random((1000, n)) * (thi - tlo)
        q = (lo - pad) + rng.random((1000, n)) * (hi - lo + 2 * pad)
        assert got <= np.linalg.norm(p - q, axis=1).min() * (1 + 1e-15)
        c = q[0]
        dist = lib.inf_set_emu_dist(n, a(c), a(tlo), a(thi))
        assert dist == T.set_dist(c, tlo, thi) and dist <= np.linalg.norm(p - c, axis=1).min() * (1 + 1e-15)
        assert lib.inf_set_emu_dist(n, a(c), a(ca), a(ca)) == I.dist(ca, c) == I.dist(c, ca)


# ------------------------------------------------------------------------------------------- refused input
def test_refused_input_returns_its_status_and_writes_nothing():
    c = I.case("boxes2")
    e = T.emu_of(c)
    tlo, thi, ptr, reg = T.batch(c, 5, "box_box", 0.3)
    cases = T.refusals(c.P, c.n, tlo, thi, ptr, reg)
    assert len(cases) == len(I.refusals(c.P, c.n, tlo, ptr, reg)) + 9
    for label, text, kind, a in cases:
        if kind == "paths":
            outs = [np.full((5, c.P), -3, np.int32), np.full(5, -3, np.int32), np.full(5, -3.0), np.full(5, -3, np.int32)]
            rc = e.raw_paths(a["B"], a["lo"], a["hi"], a["ptr"], a["reg"], a["max_len"], *outs)
        else:
            outs = [np.full((5, c.P), 7, np.uint8)]
            rc = e.raw_keep(a["B"], a["lo"], a["hi"], a["bound"], a["pad"], outs[0])
        assert rc == I.BAD_ARG, label
        assert re.search(text, e.lib.inf_set_emu_last_error().decode()), (label, e.lib.inf_set_emu_last_error())
        assert all(np.all(o == (7 if kind == "keep" else -3)) for o in outs), label
    none = np.zeros((0, 2))
    paths, cost, status = e.region_paths_sets(none, none, np.zeros(1, np.int64), np.zeros(0, np.int32))      # no query: nothing is done
    assert paths == [] and len(cost) == len(status) == 0
    assert e.informed_regions_sets(none, none, np.zeros(0)).shape == (0, c.P)
    outs = [np.full((5, c.P), -3, np.int32), np.full(5, -3, np.int32), np.full(5, -3.0), np.full(5, -3, np.int32)]
    assert e.raw_paths(5, tlo, thi, np.zeros(11, np.int64), None, c.P, *outs) == I.OK      # queries without a hit, no hit array: no path each
    assert np.all(outs[0] == -1) and np.all(outs[1] == 0) and np.all(np.isinf(outs[2])) and np.all(outs[3] == 1)


# ------------------------------------------------------------------------------------------- SceneQueries on a stand-in scene
class SetScene(InformedScene):
    """``InformedScene`` with the calls the set queries add: the two set calls through the host build, ``locate_boxes`` through the
    host build of locate_box_kernel, and the induced assembly through its host build"""

    def build_region_graph(self, flags=None):
        c = self.case
        self.sets, self.induced = T.emu_of(c), G.EmuInduced(c.P, c.row_ptr, c.tail, c.head, G.reverse_edges(c.tail, c.head))
        return InformedScene.build_region_graph(self, flags)

    def locate_boxes(self, lo, hi, tol=L.TOL):
        return bxc.emu_locate_boxes(self.polys, lo, hi, tol, n=self.n)

    def region_paths_sets(self, *a, **k):
        self.calls.append("region_paths_sets")
        return self.sets.region_paths_sets(*a, **k)

    def informed_regions_sets(self, *a, **k):
        self.calls.append("informed_regions_sets")
        return self.sets.informed_regions_sets(*a, **k)

    def induced_query_graphs(self, *a, **k):
        self.calls.append("induced_query_graphs")
        return self.induced.induced_query_graphs(*a, **k)


def box_queries(c):
    """three queries of lattice_wall as (starts or None, goals or None, start_boxes or None, goal_boxes or None), twice: point -> box and
    box -> box, the boxes of half-width 0.3 around the case's points"""
    S, G_ = c.S[:3], c.G[:3]
    sb, gb = (S - 0.3, S + 0.3), (G_ - 0.3, G_ + 0.3)
    return [dict(starts=S, goal_boxes=gb), dict(start_boxes=sb, goal_boxes=gb)]


@pytest.fixture(scope="module")
def walled():
    c = I.case("lattice_wall")
    As = {("cell", r): A for r, (A, _) in enumerate(c.polys)}; bs = {("cell", r): b for r, (_, b) in enumerate(c.polys)}
    with SceneQueries(As, bs, 2, scene=SetScene(c), pair_lp=L.PairLP()) as sq:
        yield c, sq


def test_informed_sets_on_points_is_informed(walled):
    c, sq = walled
    S, G_ = c.S[:3], c.G[:3]
    want = sq.informed(S, G_, restrict=host_restrict)
    sq.scene.calls.clear()
    got = sq.informed_sets(starts=S, goals=G_, restrict=host_restrict)
    assert sq.scene.calls == ["region_paths_sets", "informed_regions_sets"]      # one call each for the batch
    for a, b in zip(got, want):
        assert set(a) == set(b) == {"path", "bound", "keep", "restriction"}
        assert np.array_equal(a["path"], b["path"]) and a["bound"] == b["bound"] and np.array_equal(a["keep"], b["keep"])
        assert list(a["restriction"]) == list(b["restriction"]) and all(np.array_equal(a["restriction"][k], b["restriction"][k]) for k in b["restriction"])
    # a query without a bound keeps every region, though the set call takes finite bounds alone
    info = sq.informed_sets(starts=S[:2], goals=G_[:2], restrict=lambda As, bs, n, paths: [(float("inf"), None)] * len(paths))
    assert all(np.isinf(r["bound"]) and r["keep"].all() and r["restriction"] is None and len(r["path"]) > 0 for r in info)


def test_informed_sets_keeps_the_terminals_the_path_and_what_the_rule_says(walled):
    c, sq = walled
    for q in box_queries(c):
        info = sq.informed_sets(restrict=host_restrict, **q)
        points = [k for k in ("starts", "goals") if k in q]
        S, G_, regs, sb, gb = sq._located(q.get("starts"), q.get("goals"), 1e-6, 1e-9, q.get("start_boxes"), q.get("goal_boxes"))
        for i, rec in enumerate(info):
            assert len(rec["path"]) >= 1 and np.isfinite(rec["bound"])
            assert list(rec["restriction"]) == ['s'] + [("cell", int(r)) for r in rec["path"]] + ['t']
            assert np.all(rec["keep"][regs[i]]) and np.all(rec["keep"][regs[3 + i]]) and np.all(rec["keep"][rec["path"]])
            slo, shi = (S[i], S[i]) if sb is None else (sb[0][i], sb[1][i])
            want, near = T.restate_keep(c.lo, c.hi, slo, shi, gb[0][i], gb[1][i], rec["bound"] + 2.0 * len(points) * I.EPS * np.sqrt(2))
            assert not near.any()
            want[regs[i]] = want[regs[3 + i]] = True
            assert np.array_equal(rec["keep"], want)
            # the bound is a feasible path's length: at least the distance between the two sets
            assert rec["bound"] >= T.gap(slo, shi, gb[0][i][None], gb[1][i][None], 0.0)[0] - 4e-6
        assert info[0]["keep"].sum() < c.P and info[1]["keep"].sum() < c.P      # the local queries lose regions


def test_induced_assembly_equals_the_host_assembly_for_box_terminals(walled):
    c, sq = walled
    for q in box_queries(c):
        host, info = sq._graphs(q.get("starts"), q.get("goals"), 1e-6, 1e-9, "host", "informed_sets", host_restrict, q.get("start_boxes"), q.get("goal_boxes"))
        sq.scene.calls.clear()
        got = sq.graphs(prune="informed_sets", assemble="induced", restrict=host_restrict, **q)
        assert sq.scene.calls == ["region_paths_sets", "informed_regions_sets", "induced_query_graphs"]
        for i, (g, h) in enumerate(zip(got, host)):
            assert_same_graph(g, h)
            assert g.num_vertices == 2 + int(info[i]["keep"].sum())
            assert g.keys == ['s', 't'] + [sq.keys[r] for r in np.nonzero(info[i]["keep"])[0]]
        whole = sq.graphs(**q)
        assert got[0].num_vertices < whole[0].num_vertices
        # the box rows of the terminal: those of the unpruned graph
        assert got[0].poly_b[:8].tobytes() == whole[0].poly_b[:8].tobytes()


def test_the_refusals_of_prune_stay(walled):
    c, sq = walled
    q = box_queries(c)[0]
    before = list(sq.scene.calls)
    for call in (sq.graphs, sq.solve):
        with pytest.raises(ValueError, match="prune='informed' takes point terminals"):
            call(prune="informed", **q)
        with pytest.raises(ValueError, match="prune needs assemble='host'"):
            call(prune="informed_sets", assemble="device", **q)
        with pytest.raises(ValueError, match="prune must be None or 'informed'"):
            call(prune="informed_set", **q)
        with pytest.raises(ValueError, match="give exactly one of starts and start_boxes"):
            call(prune="informed_sets", goal_boxes=q["goal_boxes"])
    assert sq.scene.calls == before


# ------------------------------------------------------------------------------------------- seeded errors
# (anchor in informed_set_core.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "bound_halved": [("if (!(best < cur && best <= U)) return false;", "if (!(best < cur && best < 0.5 * U)) return false;")],
    "bound_never_lowered": [("{ return c < bound_now; }", "{ return false; }")],      # neutral: a stale bound only admits more
    "gap_from_the_low_corner": [("fmax(fmax(lo[k] - pad - thi[k], 0.0), tlo[k] - hi[k] - pad)", "fmax(fmax(lo[k] - pad - tlo[k], 0.0), tlo[k] - hi[k] - pad)")],
    "one_gap": [("return set_box_gap(q.slo, q.shi, lo, hi, n, pad) + set_box_gap(q.glo, q.ghi, lo, hi, n, pad);", "return set_box_gap(q.slo, q.shi, lo, hi, n, pad);")],
    "pad_moves_the_sides_in": [("fmax(fmax(lo[k] - pad - thi[k], 0.0), tlo[k] - hi[k] - pad)", "fmax(fmax(lo[k] + pad - thi[k], 0.0), tlo[k] - hi[k] + pad)")],
}
NEUTRAL = ("bound_never_lowered",)
SEEDED = [m for m in MUTANTS if m != "clean" and m not in NEUTRAL]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    return {name: T.declare(lib) for name, lib in build_mutants(tmp_path_factory.mktemp("informed_set_mutants"), "informed_set_core.h", MUTANTS, T.EMU_SRC).items()}


def _violations(lib):
    missed = []
    c = I.case("boxes300")
    e = T.emu_of(c, lib=lib)
    tlo, thi, ptr, reg = T.batch(c, 5, "box_box", 0.3)
    try:
        T.check_paths(e.region_paths_sets(tlo, thi, ptr, reg), c.centers, c.row_ptr, c.tail, c.head, e.w, tlo, thi, ptr, reg)
    except AssertionError:
        missed.append("paths")
    try:
        c = I.case("boxes2")
        e = T.emu_of(c, lib=lib)
        tlo, thi, ptr, reg = T.batch(c, 5, "box_box", 0.3)
        bound = np.array([3.0, 2.0, 8.0, 5.0, 6.0])
        T.check_keep(e.informed_regions_sets(tlo, thi, bound, 0.25), c.lo, c.hi, tlo, thi, bound, 0.25)
    except AssertionError:
        missed.append("keep")
    return missed


@pytest.mark.parametrize("mutant", ("clean",) + NEUTRAL)
def test_clean_copy_and_neutral_change_pass(builds, mutant):
    assert _violations(builds[mutant]) == []


def test_the_neutral_change_runs_the_search_to_the_end(builds):
    """the control is not idle: without a falling bound the local queries of boxes300 take the rounds of the point kernel"""
    c = I.case("boxes300")
    pts, ptr, reg = c.batch(2)
    e, point = T.emu_of(c, lib=builds["bound_never_lowered"]), I.emu_of(c)
    e.region_paths_sets(pts, pts, ptr, reg); point.region_paths(pts, ptr, reg)
    assert e.last[0].tobytes() == point.last[0].tobytes() and np.array_equal(e.last[1], point.last[1])


@pytest.mark.parametrize("mutant", SEEDED)
def test_seeded_errors_are_rejected(builds, mutant):
    assert _violations(builds[mutant]) == [["keep"], ["paths"]][mutant == "bound_halved"], mutant


# ------------------------------------------------------------------------------------------- the build
def test_new_kernels_are_one_each_and_use_no_scratch():
    """(no device needed: the compiler's resource remarks of the in-tree build)"""
    from gcs_admm_amd import build
    res = build.kernel_resources()
    for name in ("terminal_set_path_kernel", "terminal_set_keep_kernel"):
        mine = {k: v for k, v in res.items() if name in k}
        assert len(mine) == 1, (name, sorted(mine))
        assert all(v["scratch"] == 0 for v in mine.values()), mine
