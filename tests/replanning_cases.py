"""The replanning claim on the CPU oracle (test_replanning.py): benchmark4's regions as a scene, a query graph for any start and goal
on any subset of the regions, the oracle's loop from zero or from a state carried over by ``state_transfer_cases.transfer_reference``,
and the fixed table of second queries.  The shifts and the removed regions are also what test_gpu_state_transfer.py asks of the device."""
from __future__ import annotations

import numpy as np

import state_transfer_cases as X
from gcs_admm_amd import IPM_TOL
from gcs_admm_amd.cases import fixture_sets, load_fixture
from gcs_admm_amd.graph import convert_pt_to_polytope, graph_from_sets, polytopes_overlap, sets_of_graph
from gcs_admm_amd.rounding import rounding

NAME = "benchmark4"
# the second query: the start moved by d and the goal by -d, |d| = shift, d along DIRECTION; with and without removing regions that
# carried no flow in the base run (chosen from the base run's vertex activations, see test_replanning.py)
SHIFTS = (0.05, 0.2, 0.5)
DIRECTION = (1.0, 0.0)
REMOVED = {0.05: 0, 0.2: 3, 0.5: 6}      # regions of zero flow removed in the "removed" rows, as in the issue's table
# a region carried no flow: its activation y_v at the base run's stop is below this -- ten times eps_abs, the loop's absolute stop
# tolerance, under which an activation is not told from zero (the regions of the path have y_v near 1)
NO_FLOW = 1e-3


class Scene:
    """benchmark4's regions with the region-region edges of its fixture; the terminals come with each query"""

    def __init__(self, name=NAME):
        As, bs, n, _, _ = fixture_sets(name)
        _, g = load_fixture(name)
        self.n = n
        self.region_keys = [k for k in g.keys if k not in ('s', 't')]
        self.As, self.bs = {k: As[k] for k in self.region_keys}, {k: bs[k] for k in self.region_keys}
        self.region_edges = [(u, w) for u, w in g.edges_as_keys() if u not in ('s', 't') and w not in ('s', 't')]
        self.serial = {k: i for i, k in enumerate(self.region_keys)}
        self.s, self.t = g.interior[g.src].copy(), g.interior[g.dst].copy()

    def graph(self, s, t, removed=()):
        """(graph, vertex ids) of the query (s, t) on the regions that are not ``removed``: keys ['s', 't', *regions], the terminals'
        edges by ``graph.polytopes_overlap``, the edge list ascending in (tail, head)"""
        gone = set(removed)
        keys = [k for k in self.region_keys if k not in gone]
        As, bs = {}, {}
        As['s'], bs['s'] = convert_pt_to_polytope(np.asarray(s, float), 1e-6)
        As['t'], bs['t'] = convert_pt_to_polytope(np.asarray(t, float), 1e-6)
        edges = [(u, w) for u, w in self.region_edges if u not in gone and w not in gone]
        for term in ('s', 't'):
            hits = [k for k in keys if polytopes_overlap(As[term], bs[term], self.As[k], self.bs[k])]
            if not hits:
                raise ValueError(f"{term} lies in no region")
            edges += [(term, k) for k in hits] + [(k, term) for k in hits]
        for k in keys:
            As[k], bs[k] = self.As[k], self.bs[k]
        index = {k: i for i, k in enumerate(['s', 't'] + keys)}
        edges.sort(key=lambda e: (index[e[0]], index[e[1]]))
        g = graph_from_sets(As, bs, self.n, edges=edges)
        assert g.keys[:2] == ['s', 't']
        return g, np.array([0, 1] + [self.serial[k] + 2 for k in keys], np.int32)

    def solve(self, s, t, removed=(), seed=None):
        """the oracle's loop on the query, default parameters, from zero or (``seed``: the record of an earlier ``solve``) from that
        run's final state carried over by ``transfer_reference``, the warm-start records of the vertex solves cleared either way.
        The record: iterations, cost (relaxed), rounded_cost, flow (activation per region key) and what a later seed needs."""
        from oracle import oracle as O
        g, ids = self.graph(s, t, removed)
        o = O.Oracle(g, ipm_tol=IPM_TOL)
        side = X.Side(g, ids, "incidence", "f64", fill="zero")
        if seed is not None:
            for k, a in X.transfer_reference(seed["side"], side).items():
                getattr(o, k)[...] = a
        res = o.run(nthreads=4)
        rho = res["rho_seq"]
        side.state = {k: getattr(o, k).copy() for k in X.STATE}
        side.rho, side.mu_scale = float(rho[-1]), float(rho[-2] / rho[-1])      # the rescale the last control step left pending
        V, E, n = g.keys, g.edges_as_keys(), self.n
        y_e = {e: float(o.zedge[2 * n, i]) for i, e in enumerate(E)}
        As, bs = sets_of_graph(g)
        cost, _, _ = rounding(y_e, V, E, {v: [e for e in E if e[0] == v] for v in V}, As, bs, n)
        return dict(iterations=int(res["iterations"]), status=res["status"], cost=float(res["cost"]), rounded_cost=float(cost), graph=g, side=side,
                    flow={k: float(o.yv[i]) for i, k in enumerate(g.keys)})


def no_flow_regions(record, count):
    """``count`` regions of the record's graph with the smallest activation, all below NO_FLOW, in scene order"""
    quiet = sorted((v, k) for k, v in record["flow"].items() if k not in ('s', 't'))[:count]
    assert all(v < NO_FLOW for v, _ in quiet), quiet
    return [k for _, k in quiet]


def queries(scene, base):
    """(label, start, goal, removed regions) of the fixed table: every shift without and -- where REMOVED says so -- with removal"""
    d = np.asarray(DIRECTION)
    for shift in SHIFTS:
        yield f"shift{shift}", scene.s + shift * d, scene.t - shift * d, []
        if REMOVED[shift]:
            yield f"shift{shift}-removed{REMOVED[shift]}", scene.s + shift * d, scene.t - shift * d, no_flow_regions(base, REMOVED[shift])
