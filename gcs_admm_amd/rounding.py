"""Rounding of the relaxed edge activations to an s-t path and the convex restriction along it --
the step that follows the ADMM loop in the reference (GCS_utils.py:92-181 ``rounding``,
:17-89 ``solve_convex_restriction``; called at admm_solver_v3.py:759 with N=5, M=20, the case file's
own N, M being ignored -- quirk Q5).  SURVEY.md section 8(f) item 1; runs once, on the host by default.
``restriction="device"`` solves all candidate paths side by side on the MI355X (csrc/path_restrict_core.h
through ``gcsadmm_scene_restrict_paths``), and ``rounding_many`` does the same for the candidates of many
problems in one call per round.  In ``rounding`` and ``rounding_many`` the walk runs on the host, on one dict
entry per edge; ``rounding_members`` draws the walks of all members of a batch on the device instead
(``walks.DeviceWalks``, csrc/path_walk_core.h: a rule of its own with a counter-based generator, not the host's
draws) and builds no per-edge Python object.

Differences from the reference, on purpose: the random walk is seeded (the reference draws from the
unseeded global numpy generator, GCS_utils.py:131, so its runs are not reproducible), and the
restriction is solved by this repo's own small SOCP solver (gcs_admm_amd/conic.py) on the polyline
form: along a fixed path the continuity constraints x_{v,2} = x_{w,1} make the unknowns a chain of
points q_0 .. q_{k+1} with q_j, q_{j+1} in P_{v_j}, and the cost is the polyline length.
"""
from __future__ import annotations

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
    k = len(path)
    # point j lies in P_{path[j-1]} and P_{path[j]} (ends: only one region)
    regions = [[path[0]]] + [[path[j - 1], path[j]] for j in range(1, k)] + [[path[-1]]]
    npts = k + 1
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


class _Candidates:
    """The candidate paths of ``rounding`` in the order the host loop visits them, handed out in rounds: the most probable path,
    then seeded walks until N distinct paths are feasible or pending, or M draws are spent.  When a round comes back with
    infeasible paths the next one goes on drawing with the remaining draws -- the draws and the list are the host loop's."""

    def __init__(self, y_e_sol, I_v_out, N, M, seed):
        self.y_e, self.I_out, self.N, self.draws_left = y_e_sol, I_v_out, N, M
        self.rng = np.random.default_rng(seed)
        self.seen, self.cands, self.started = set(), [], False

    def next_round(self):
        pending = []
        if not self.started:
            self.started = True
            first = most_probable_path(self.y_e, self.I_out)
            if first is not None:
                self.seen.add(tuple(first)); pending.append(first)
        while self.draws_left > 0 and len(self.cands) + len(pending) < self.N:
            self.draws_left -= 1
            pth = find_path_via_random_dfs(self.y_e, self.I_out, self.rng)
            if pth is None or tuple(pth) in self.seen:
                continue
            self.seen.add(tuple(pth)); pending.append(pth)
        return pending

    def take(self, pending, results):
        self.cands += [(cost, pth, xs) for pth, (cost, xs) in zip(pending, results) if xs is not None]


def _rounded(cands, V, n):
    cands = [c for c in cands if np.isfinite(c[0])]        # (a failed solve was a candidate of the walk, never a result)
    if not cands:
        print("Rounding failed to find any feasible paths.")
        return float('inf'), None, None
    cost, pth, xs = min(cands, key=lambda t: t[0])
    return cost, {v: xs.get(v, np.zeros(2 * n)) for v in V}, {v: (1 if v in xs else 0) for v in V}


def rounding_many(problems, N=5, M=20, device=0, solver=None):
    """``rounding(..., restriction="device")`` for many problems at once (the members of a ``BatchSolver``, for instance):
    ``problems`` is a list of dicts with the arguments of ``rounding`` (``y_e_sol, V, E, I_v_out, As, bs, n`` and optionally
    ``seed``), all of one dimension n.  The candidates of every problem are solved in ONE call per round, on one scene over the
    concatenated regions.  Returns the list of ``(cost, x_v_rounded, y_v_rounded)``, each exactly what ``rounding`` returns for
    that problem alone.  ``solver``: as in ``rounding``, on the concatenated regions (keys ``(problem index, region key)``)."""
    if not problems:
        return []
    n = problems[0]["n"]
    if any(pr["n"] != n for pr in problems):
        raise ValueError("rounding_many needs problems of one dimension n")
    As = {(i, v): pr["As"][v] for i, pr in enumerate(problems) for v in pr["As"]}
    bs = {(i, v): pr["bs"][v] for i, pr in enumerate(problems) for v in pr["As"]}
    scene = None
    if solver is None:
        from .scene import DeviceScene
        scene = DeviceScene([(np.asarray(As[k], float), np.asarray(bs[k], float)) for k in As], device)
        solver = lambda As_, bs_, n_, paths: solve_path_restrictions_device(As_, bs_, n_, paths, device, scene)
    try:
        gens = [_Candidates(pr["y_e_sol"], pr["I_v_out"], N, M, pr.get("seed", 0)) for pr in problems]
        _solve_rounds(gens, As, bs, n, solver)
    finally:
        if scene is not None:
            scene.close()
    return [_rounded(g.cands, pr["V"], n) for g, pr in zip(gens, problems)]


def _solve_rounds(gens, As, bs, n, solver):
    """round after round of the candidate generators of many problems, each round's paths in ONE ``solver`` call on the concatenated
    regions (keys ``(problem index, region key)``), until no generator has a path left"""
    while True:
        rounds = [g.next_round() for g in gens]
        if not any(rounds):
            break
        results = solver(As, bs, n, [[(i, v) for v in pth] for i, pend in enumerate(rounds) for pth in pend])
        at = 0
        for g, pend in zip(gens, rounds):
            mine = [(cost, None if xs is None else {k[1]: x for k, x in xs.items()}) for cost, xs in results[at:at + len(pend)]]
            g.take(pend, mine)
            at += len(pend)


class _DrawnCandidates:
    """``_Candidates`` on walks that are drawn already (``paths[w]``, ``status[w]`` of walks 0 .. M, by vertex key): the same
    accounting -- walk 0 first, then draws 1 .. M in order, a draw spent on every walk looked at, dead ends, overruns and duplicates
    skipped, at most N paths feasible or pending, and drawing goes on after a round with infeasible paths."""

    def __init__(self, paths, status, N, M):
        self.paths, self.status, self.N, self.M = paths, status, N, min(M, len(paths) - 1)
        self.next, self.seen, self.cands = 0, set(), []

    def next_round(self):
        pending = []
        while self.next <= self.M and (self.next == 0 or len(self.cands) + len(pending) < self.N):
            w, self.next = self.next, self.next + 1
            pth = self.paths[w]
            if self.status[w] != 0 or tuple(pth) in self.seen:
                continue
            self.seen.add(tuple(pth)); pending.append(pth)
        return pending

    def take(self, pending, results):
        self.cands += [(cost, pth, xs) for pth, (cost, xs) in zip(pending, results) if xs is not None]


def device_sampler(device=0):
    """the sampler of ``rounding_members``: walks 0 .. count - 1 of every member from ONE ``DeviceWalks.sample`` call on the members'
    activation rows ``zedge[2 n]``, where the solver left them"""
    def sample(members, graphs, seeds, count):
        from .walks import DeviceWalks
        with DeviceWalks(graphs, device) as walks:
            return walks.sample([m.zedge[2 * g.n] for m, g in zip(members, graphs)], seeds, 0, count)
    return sample


def rounding_members(members, graphs, N=5, M=20, seeds=None, device=0, sampler=None, solver=None):
    """The rounding step for the members of a batch with the walks drawn on the device: ``members[i]`` is the solver that has just run
    ``graphs[i]`` (its activations are read on the device; nothing per edge comes to the host), all of one dimension n.
    ``sampler(members, graphs, seeds, count) -> [(paths, status)]`` per member, paths as arrays of vertex indices (default:
    ``device_sampler(device)``), is called ONCE, for walks 0 .. M.  The candidates of a member are its walk 0 and then its draws
    1 .. M in order, without dead ends, overruns and duplicates, at most N feasible or pending at any time, as in ``rounding``; the
    restrictions go through ``solver`` (as in ``rounding_many``: default ``solve_path_restrictions_device`` on one scene over the
    concatenated regions), one call per round for all members.  Returns ``(cost, x_v_rounded, y_v_rounded)`` per member, in the
    shape of ``rounding``; a member without a successful walk gives ``(inf, None, None)``.

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
    gens = [_DrawnCandidates([[g.keys[v] for v in pth] for pth in paths], status, N, M) for g, (paths, status) in zip(graphs, drawn)]
    As, bs = {}, {}
    for i, g in enumerate(graphs):      # per vertex: views into the graph's polytope CSR
        A_i, b_i = sets_of_graph(g)
        As.update(((i, v), A) for v, A in A_i.items()); bs.update(((i, v), b) for v, b in b_i.items())
    scene = None
    if solver is None:
        from .scene import DeviceScene
        scene = DeviceScene([(np.asarray(As[k], float), np.asarray(bs[k], float)) for k in As], device)
        solver = lambda As_, bs_, n_, paths: solve_path_restrictions_device(As_, bs_, n_, paths, device, scene)
    try:
        _solve_rounds(gens, As, bs, n, solver)
    finally:
        if scene is not None:
            scene.close()
    return [_rounded(gen.cands, g.keys, n) for gen, g in zip(gens, graphs)]


def rounding(y_e_sol, V, E, I_v_out, As, bs, n, N=5, M=20, seed=0, restriction="host", solver=None, device=0):
    """Up to M seeded random walks, at most N distinct paths, best restricted cost wins
    (GCS_utils.py:148-181); the deterministic most-probable path is tried first (an addition: it
    removes most of the run-to-run variation the reference's unseeded sampling has).  Returns
    (cost, x_v_rounded, y_v_rounded) with the reference's shapes: every vertex has an entry;
    off-path vertices get x = 0, y = 0.

    ``restriction``: ``"host"`` (the default: one ``solve_path_restriction`` after the other, as before) or ``"device"``: the
    same candidates from the same draws, collected first and solved in one call of ``solver(As, bs, n, paths) -> [(cost, xs)]``
    (default ``solve_path_restrictions_device`` on ``device``); when paths come back infeasible, drawing goes on with the
    remaining draws, so that for one seed the candidate list is the host's."""
    if restriction not in ("host", "device"):
        raise ValueError(f"restriction must be 'host' or 'device', not {restriction!r}")
    if restriction == "device":
        if solver is None:
            solver = lambda As_, bs_, n_, paths: solve_path_restrictions_device(As_, bs_, n_, paths, device)
        gen = _Candidates(y_e_sol, I_v_out, N, M, seed)
        while True:
            pending = gen.next_round()
            if not pending:
                break
            gen.take(pending, solver(As, bs, n, pending))
        return _rounded(gen.cands, V, n)
    rng = np.random.default_rng(seed)
    seen, cands = set(), []
    first = most_probable_path(y_e_sol, I_v_out)
    if first is not None:
        seen.add(tuple(first))
        cost, xs = solve_path_restriction(As, bs, n, first)
        if xs is not None:
            cands.append((cost, first, xs))
    for _ in range(M):
        if len(cands) >= N:
            break
        pth = find_path_via_random_dfs(y_e_sol, I_v_out, rng)
        if pth is None or tuple(pth) in seen:
            continue
        seen.add(tuple(pth))
        cost, xs = solve_path_restriction(As, bs, n, pth)
        if xs is not None:
            cands.append((cost, pth, xs))
    if not cands:
        print("Rounding failed to find any feasible paths.")
        return float('inf'), None, None
    cost, pth, xs = min(cands, key=lambda t: t[0])
    x_v = {v: xs.get(v, np.zeros(2 * n)) for v in V}
    y_v = {v: (1 if v in xs else 0) for v in V}
    return cost, x_v, y_v
