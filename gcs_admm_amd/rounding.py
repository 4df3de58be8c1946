"""Rounding of the relaxed edge activations to an s-t path and the convex restriction along it --
the step that follows the ADMM loop in the reference (GCS_utils.py:92-181 ``rounding``,
:17-89 ``solve_convex_restriction``; called at admm_solver_v3.py:759 with N=5, M=20, the case file's
own N, M being ignored -- quirk Q5).  SURVEY.md section 8(f) item 1; runs once, on the host by default.

Every entry point is the same three pieces.  The candidate rule (``_Candidates``: walk 0, then up to M draws, dead ends and
duplicates skipped, at most N paths feasible or pending) over an iterator of walks; the round loop (``_solve_rounds``: the pending
paths of all problems in one solver call per round); the result rule (``_rounded``: the cheapest candidate of finite cost).  They
differ in where walks and solves come from.  ``rounding``: host walks (``_host_walks``: lazy, seeded, one dict entry per edge),
solved by ``solve_path_restriction`` one after the other (``restriction="host"``) or side by side on the MI355X
(``"device"``: csrc/path_restrict_core.h through ``gcsadmm_scene_restrict_paths``).  ``rounding_many``: host walks of many
problems, solved on one scene over the concatenated regions.  ``rounding_members``: the same, on walks that the device has drawn
for all members of a batch in one call (``_drawn_walks`` on ``walks.DeviceWalks``, csrc/path_walk_core.h: a rule of its own with a
counter-based generator, not the host's draws), with no per-edge Python object.

Differences from the reference, on purpose: the random walk is seeded (the reference draws from the
unseeded global numpy generator, GCS_utils.py:131, so its runs are not reproducible), and the
restriction is solved by this repo's own small SOCP solver (gcs_admm_amd/conic.py) on the polyline
form: along a fixed path the continuity constraints x_{v,2} = x_{w,1} make the unknowns a chain of
points q_0 .. q_{k+1} with q_j, q_{j+1} in P_{v_j}, and the cost is the polyline length.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np

from .conic import solve_socp
from .graph import chebyshev_center


def find_path_via_random_dfs(y_e: Dict[Tuple[Hashable, Hashable], float], I_v_out, rng) -> Optional[List[Hashable]]:
    """Walk from 's' choosing the next out-edge with probability proportional to y_e (edges with y_e <= 1e-15 and visited heads
    excluded), one draw per node.  The reference writes this as a recursive depth-first search (GCS_utils.py:109-146) in which a
    node draws ONCE and, when the branch below it fails, backs out and reports failure itself: a dead end anywhere unwinds the whole
    walk.  The same thing as a loop (no recursion limit on paths through thousands of regions)."""
    path, visited, cur = ['s'], {'s'}, 's'
    while cur != 't':
        edges = [e for e in I_v_out.get(cur, []) if e[1] not in visited and y_e.get(e, 0) > 1e-15]
        if not edges:
            return None
        probs = np.array([y_e[e] for e in edges], dtype=float)
        tot = probs.sum()
        if tot < 1e-15:
            return None
        idx = int(np.searchsorted(np.cumsum(probs / tot), rng.random()))
        cur = edges[min(idx, len(edges) - 1)][1]
        visited.add(cur); path.append(cur)
    return path


def solve_path_restriction(As, bs, n: int, path: Sequence[Hashable]):
    """Shortest polyline through the regions of ``path`` in order.  Returns (cost, {v: x_v (2n)})
    or (inf, None) when consecutive regions do not intersect."""
    regions = path_point_regions(path)
    npts = len(path) + 1
    q0 = []
    for reg in regions:
        A = np.vstack([np.asarray(As[v], float) for v in reg]); b = np.hstack([np.asarray(bs[v], float) for v in reg])
        try:
            q0.append(chebyshev_center(A, b))
        except ValueError:
            return float('inf'), None
    nseg = npts - 1
    nw = npts * n + nseg                       # points, then one epigraph variable per segment
    c = np.zeros(nw); c[npts * n:] = 1.0
    rows, rhs = [], []
    for j, reg in enumerate(regions):
        for v in reg:
            A = np.asarray(As[v], float); b = np.asarray(bs[v], float)
            for r in range(A.shape[0]):
                row = np.zeros(nw); row[j * n:(j + 1) * n] = A[r]
                rows.append(row); rhs.append(b[r])
    p = len(rows)
    for sgm in range(nseg):                    # cone: (t_s, q_{s+1} - q_s)
        row = np.zeros(nw); row[npts * n + sgm] = -1.0
        rows.append(row); rhs.append(0.0)
        for d in range(n):
            row = np.zeros(nw); row[(sgm + 1) * n + d] = -1.0; row[sgm * n + d] = 1.0
            rows.append(row); rhs.append(0.0)
    w0 = np.concatenate([np.concatenate(q0)] + [[np.linalg.norm(q0[s + 1] - q0[s]) + 1.0] for s in range(nseg)])
    w, val, _ = solve_socp(c, np.array(rows), np.array(rhs), p, [n + 1] * nseg, w0)
    q = w[:npts * n].reshape(npts, n)
    cost = float(sum(np.linalg.norm(q[s + 1] - q[s]) for s in range(nseg)))
    return cost, {v: np.concatenate([q[j], q[j + 1]]) for j, v in enumerate(path)}


def most_probable_path(y_e, I_v_out) -> Optional[List[Hashable]]:
    """Deterministic walk that always takes the out-edge with the largest activation."""
    path, visited, cur = ['s'], {'s'}, 's'
    while cur != 't':
        cand = [(y_e.get(e, 0.0), k) for k, e in enumerate(I_v_out.get(cur, [])) if e[1] not in visited and y_e.get(e, 0) > 1e-15]
        if not cand:
            return None
        cur = I_v_out[cur][max(cand)[1]][1]
        visited.add(cur); path.append(cur)
    return path


def path_point_regions(path):
    """regions of every point of the polyline along ``path``: point j lies in path[j-1] and path[j] (the ends: in one region)"""
    k = len(path)
    return [(path[0],)] + [(path[j - 1], path[j]) for j in range(1, k)] + [(path[-1],)]


def solve_path_restrictions(As, bs, n, paths, centers, restrict):
    """``solve_path_restriction`` for many paths at once, on injected callables (tests run this logic without a GPU):
    ``centers(polys) -> (centres, radii, status)`` are the Chebyshev-centre LPs of a list of polytopes, ``restrict(polys, paths,
    starts) -> (points, cost, iterations, status)`` the restriction along paths of INDICES into ``polys`` (the contract of
    ``DeviceScene.restrict_paths``).  The start points are the centres of the distinct one- or two-region intersections, from ONE
    call of ``centers``; a radius <= 0 or a failed LP makes the path infeasible without solving it.  Returns ``(cost, xs)`` per
    path in the shape of ``solve_path_restriction``; an infeasible path (no start, or status 1) gives ``(inf, None)``.  A solve
    that FAILED (status -1: iteration limit, vanished step) says nothing about feasibility: it gives ``(inf, xs)`` with its last
    iterate, so that the caller counts the path as visited, as the host loop does with whatever its solver returns, but never
    prefers it."""
    keys = list(As)
    index = {v: i for i, v in enumerate(keys)}
    polys = [(np.asarray(As[v], float), np.asarray(bs[v], float)) for v in keys]
    inter = {}
    for path in paths:
        for reg in path_point_regions(path):
            inter.setdefault(reg, len(inter))
    out = [(float('inf'), None)] * len(paths)
    if not inter:
        return out
    cen, rad, st = centers([(np.vstack([polys[index[v]][0] for v in reg]), np.hstack([polys[index[v]][1] for v in reg])) for reg in inter])
    usable = (np.asarray(st) >= 0) & (np.asarray(rad) > 0)
    live, starts = [], []
    for p, path in enumerate(paths):
        ids = [inter[reg] for reg in path_point_regions(path)]
        if all(usable[i] for i in ids):
            live.append(p); starts.append(np.asarray(cen)[ids])
    if live:
        pts, cost, _, status = restrict(polys, [[index[v] for v in paths[p]] for p in live], starts)
        for i, p in enumerate(live):
            if status[i] <= 0:
                q = np.asarray(pts[i])
                out[p] = (float(cost[i]) if status[i] == 0 else float('inf'), {v: np.concatenate([q[j], q[j + 1]]) for j, v in enumerate(paths[p])})
    return out


def solve_path_restrictions_device(As, bs, n, paths, device=0, scene=None):
    """``(cost, xs)`` of ``solve_path_restriction`` for every path of ``paths``, solved side by side on the device: the start
    points from one call of the centre LPs on a temporary scene of the distinct intersections, the restrictions from one call
    of ``gcsadmm_scene_restrict_paths``.  ``scene``: a ``DeviceScene`` of the regions in the order of ``As`` (left open), so that
    many calls reuse one upload.  There is no CPU fallback."""
    from .scene import DeviceScene, PolytopeScene
    own = scene is None

    def restrict(polys, idx_paths, starts):
        nonlocal scene
        if scene is None:
            scene = DeviceScene(polys, device)
        return scene.restrict_paths(idx_paths, starts)
    try:
        return solve_path_restrictions(As, bs, n, paths, lambda polys: PolytopeScene(polys, device).centers(), restrict)
    finally:
        if own and scene is not None:
            scene.close()


def rounding_problem(dev, As, bs, seed=0):
    """The arguments of ``rounding`` (one entry of ``rounding_many``'s ``problems``) for the problem solver ``dev`` has just run: the
    relaxed edge activations y_e off its edge words, by edge key, and the out-lists in edge order (reference utils.py:75-80)."""
    g = dev.g
    V, E = g.keys, g.edges_as_keys()
    ye = dev.zedge[2 * g.n].cpu().numpy()
    I_v_out = {v: [] for v in V}
    for e in E:
        I_v_out[e[0]].append(e)
    return dict(y_e_sol={e: float(ye[i]) for i, e in enumerate(E)}, V=V, E=E, I_v_out=I_v_out, As=As, bs=bs, n=g.n, seed=seed)


def _host_walks(y_e_sol, I_v_out, M, seed):
    """walk 0 (the most probable path), then the M seeded draws, each made only when it is asked for; a dead end is ``None``"""
    yield most_probable_path(y_e_sol, I_v_out)
    rng = np.random.default_rng(seed)
    for _ in range(M):
        yield find_path_via_random_dfs(y_e_sol, I_v_out, rng)


def _drawn_walks(paths, status, keys, M):
    """walks 0 .. M that are drawn already (``paths[w]`` of vertex indices, ``status[w]``), by vertex key; a dead end or an overrun is
    ``None``"""
    for w in range(min(M, len(paths) - 1) + 1):
        yield [keys[v] for v in paths[w]] if status[w] == 0 else None


class _Candidates:
    """THE candidate rule of the rounding step, over an iterator of walks (walk 0 first, then the draws; a path or ``None``), handed
    out in rounds: walk 0 whatever N is, then draws while fewer than N distinct paths are feasible or pending; every walk looked at is
    spent, dead ends and duplicates are skipped.  When a round comes back with infeasible paths the next one goes on with the
    remaining draws, so the paths are those of a loop that solves each one before it draws the next."""

    def __init__(self, walks, N):
        self.walks, self.N = walks, N
        self.seen, self.cands, self.started = set(), [], False

    def next_round(self):
        pending = []
        while not self.started or len(self.cands) + len(pending) < self.N:
            self.started = True
            try:
                pth = next(self.walks)
            except StopIteration:
                break
            if pth is not None and tuple(pth) not in self.seen:
                self.seen.add(tuple(pth)); pending.append(pth)
        return pending

    def take(self, pending, results):
        self.cands += [(cost, pth, xs) for pth, (cost, xs) in zip(pending, results) if xs is not None]


def _solve_rounds(cands, solve):
    """round after round of the candidates of many problems, each round's paths in ONE call ``solve([(problem index, path)]) ->
    [(cost, xs)]``, until no problem has a path left"""
    while True:
        rounds = [c.next_round() for c in cands]
        if not any(rounds):
            return
        results = iter(solve([(i, pth) for i, pend in enumerate(rounds) for pth in pend]))
        for c, pend in zip(cands, rounds):
            c.take(pend, [next(results) for _ in pend])


def _rounded(cands, V, n):
    cands = [c for c in cands if np.isfinite(c[0])]        # (a failed solve was a candidate of the walk, never a result)
    if not cands:
        print("Rounding failed to find any feasible paths.")
        return float('inf'), None, None
    cost, pth, xs = min(cands, key=lambda t: t[0])
    return cost, {v: xs.get(v, np.zeros(2 * n)) for v in V}, {v: (1 if v in xs else 0) for v in V}


def rounding_many(problems, N=5, M=20, device=0, solver=None, extra=None):
    """``rounding(..., restriction="device")`` for many problems at once (the members of a ``BatchSolver``, for instance):
    ``problems`` is a list of dicts with the arguments of ``rounding`` (``y_e_sol, V, E, I_v_out, As, bs, n`` and optionally
    ``seed``), all of one dimension n.  The candidates of every problem are solved in ONE call per round, on one scene over the
    concatenated regions.  Returns the list of ``(cost, x_v_rounded, y_v_rounded)``, each exactly what ``rounding`` returns for
    that problem alone.  ``solver``: as in ``rounding``, on the concatenated regions (keys ``(problem index, region key)``).
    ``extra``: per problem a list of candidates ``(cost, path, xs)`` that are solved already (``xs`` by vertex key, as ``solver``
    returns them); they join the problem's candidates under the result rule, beside the N paths of the walks."""
    if not problems:
        return []
    n = problems[0]["n"]
    if any(pr["n"] != n for pr in problems):
        raise ValueError("rounding_many needs problems of one dimension n")
    As = {(i, v): pr["As"][v] for i, pr in enumerate(problems) for v in pr["As"]}
    bs = {(i, v): pr["bs"][v] for i, pr in enumerate(problems) for v in pr["As"]}
    cands = [_Candidates(_host_walks(pr["y_e_sol"], pr["I_v_out"], M, pr.get("seed", 0)), N) for pr in problems]
    return _round_batch(cands, [pr["V"] for pr in problems], As, bs, n, device, solver, extra)


@contextlib.contextmanager
def _scene_solver(As, bs, device, solver=None):
    """``solver``, or in its absence the device solver on ONE scene of the regions in the order of ``As``, open for the block"""
    if solver is not None:
        yield solver
        return
    from .scene import DeviceScene
    with contextlib.closing(DeviceScene([(np.asarray(As[k], float), np.asarray(bs[k], float)) for k in As], device)) as scene:
        yield lambda As_, bs_, n_, paths: solve_path_restrictions_device(As_, bs_, n_, paths, device, scene)


def _round_batch(cands, Vs, As, bs, n, device, solver, extra=None):
    """the rounds of many problems on their concatenated regions ``As``, ``bs`` (keys ``(problem index, region key)``: the solver gets
    paths of such keys, the candidates get their points back by region key), and every problem's result; ``extra``: as ``rounding_many``"""
    with _scene_solver(As, bs, device, solver) as run:
        def solve(jobs):
            results = run(As, bs, n, [[(i, v) for v in pth] for i, pth in jobs])
            return [(cost, None if xs is None else {k[1]: x for k, x in xs.items()}) for cost, xs in results]
        _solve_rounds(cands, solve)
    extra = extra or [[]] * len(cands)
    return [_rounded(c.cands + list(more), V, n) for c, V, more in zip(cands, Vs, extra)]


def device_sampler(device=0):
    """the sampler of ``rounding_members``: walks 0 .. count - 1 of every member from ONE ``DeviceWalks.sample`` call on the members'
    activation rows ``zedge[2 n]``, where the solver left them"""
    def sample(members, graphs, seeds, count):
        from .walks import DeviceWalks
        with DeviceWalks(graphs, device) as walks:
            return walks.sample([m.zedge[2 * g.n] for m, g in zip(members, graphs)], seeds, 0, count)
    return sample


def rounding_members(members, graphs, N=5, M=20, seeds=None, device=0, sampler=None, solver=None, extra=None):
    """The rounding step for the members of a batch with the walks drawn on the device: ``members[i]`` is the solver that has just run
    ``graphs[i]`` (its activations are read on the device; nothing per edge comes to the host), all of one dimension n.
    ``sampler(members, graphs, seeds, count) -> [(paths, status)]`` per member, paths as arrays of vertex indices (default:
    ``device_sampler(device)``), is called ONCE, for walks 0 .. M.  The candidates of a member are its walk 0 and then its draws
    1 .. M in order, without dead ends, overruns and duplicates, at most N feasible or pending at any time, as in ``rounding``; the
    restrictions go through ``solver`` (as in ``rounding_many``: default ``solve_path_restrictions_device`` on one scene over the
    concatenated regions), one call per round for all members.  Returns ``(cost, x_v_rounded, y_v_rounded)`` per member, in the
    shape of ``rounding``; a member without a successful walk gives ``(inf, None, None)``.  ``extra``: as ``rounding_many``.

    The walks follow the rule of ``walks.walk_reference``, not the host generator's draws: for one seed the candidates differ from
    those of ``rounding``.  An activation below 2^-40 counts as absent (the host walk: 1e-15)."""
    from .graph import sets_of_graph
    if not graphs:
        return []
    if len(members) != len(graphs):
        raise ValueError("one graph per member")
    n = graphs[0].n
    if any(g.n != n for g in graphs):
        raise ValueError("rounding_members needs problems of one dimension n")
    seeds = [0] * len(graphs) if seeds is None else list(seeds)
    if len(seeds) != len(graphs):
        raise ValueError("one seed per member")
    drawn = (sampler or device_sampler(device))(members, graphs, seeds, M + 1)
    cands = [_Candidates(_drawn_walks(paths, status, g.keys, M), N) for g, (paths, status) in zip(graphs, drawn)]
    As, bs = {}, {}
    for i, g in enumerate(graphs):      # per vertex: views into the graph's polytope CSR
        A_i, b_i = sets_of_graph(g)
        As.update(((i, v), A) for v, A in A_i.items()); bs.update(((i, v), b) for v, b in b_i.items())
    return _round_batch(cands, [g.keys for g in graphs], As, bs, n, device, solver, extra)


def rounding(y_e_sol, V, E, I_v_out, As, bs, n, N=5, M=20, seed=0, restriction="host", solver=None, device=0):
    """Up to M seeded random walks, at most N distinct paths, best restricted cost wins
    (GCS_utils.py:148-181); the deterministic most-probable path is tried first (an addition: it
    removes most of the run-to-run variation the reference's unseeded sampling has).  Returns
    (cost, x_v_rounded, y_v_rounded) with the reference's shapes: every vertex has an entry;
    off-path vertices get x = 0, y = 0.

    The candidates come in rounds (``_Candidates``), each round solved in one call of ``solver(As, bs, n, paths) -> [(cost, xs)]``;
    when paths come back infeasible, drawing goes on with the remaining draws, so that for one seed the paths are those of a loop
    that solves one after the other.  ``restriction``: ``"host"`` (the default: ``solve_path_restriction`` path by path, whatever
    ``solver`` is) or ``"device"`` (``solver``, default ``solve_path_restrictions_device`` on ``device``)."""
    if restriction not in ("host", "device"):
        raise ValueError(f"restriction must be 'host' or 'device', not {restriction!r}")
    if restriction == "host":
        solver = lambda As_, bs_, n_, paths: [solve_path_restriction(As_, bs_, n_, p) for p in paths]
    elif solver is None:
        solver = lambda As_, bs_, n_, paths: solve_path_restrictions_device(As_, bs_, n_, paths, device)
    cands = _Candidates(_host_walks(y_e_sol, I_v_out, M, seed), N)
    _solve_rounds([cands], lambda jobs: solver(As, bs, n, [pth for _, pth in jobs]))
    return _rounded(cands.cands, V, n)
