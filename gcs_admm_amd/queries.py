"""Many start / goal queries on one scene: the use case ``batch.py`` names for ``BatchSolver``.

A query differs from the next one only in its two terminals, so the region graph -- the centre LPs, the box LPs, the sweep and every
region-region overlap LP -- is decided ONCE, on a resident ``DeviceScene``.  Per call, ``locate_kernel`` (csrc/point_locate_core.h)
lists the regions under every start and goal point; only hits in the band of about 1e-6 around a facet or a vertex go to a pair LP,
all of them in one call.  The query graphs are the region graph plus the terminals' edges, in the order and with the arrays a
from-scratch ``graph_from_sets_device`` on ``{'s', 't', regions}`` gives; ``solve`` takes them through ``BatchSolver`` and
``rounding_many``.  By default the graphs are assembled on the host (a sort over all edges per query); ``assemble="device"`` takes them
from one kernel call on the scene's own region graph (csrc/query_graph_core.h), the same arrays.  The scene is not frozen: ``add_regions`` and ``remove_regions`` edit it in place, and only the LPs of what is new run.  There is no CPU fallback: the LPs and the locate call run on the device (tests inject stand-ins).
"""
from __future__ import annotations

import contextlib
from typing import Dict, Hashable

import numpy as np

from .graph import GcsGraph, _finish_graph, convert_pt_to_polytope, polytopes_overlap

__all__ = ["SceneQueries"]

IN, UNDECIDED = 1, 2      # hit classes of gcsadmm_scene_locate_points


class SceneQueries:
    """``As``, ``bs``: the regions alone, by key (a key ``'s'`` or ``'t'`` is refused: the terminals come with each query).  Opens one
    ``DeviceScene`` and decides the region graph on it; release with ``close()`` or use as a context manager.

    ``scene``: a prepared scene with the interface of ``DeviceScene`` (tests inject one; it is closed with the object).  ``pair_lp``:
    ``(polys, pair_a, pair_b, tol, centers) -> (flags, status)``, the pair LPs of ``PolytopeScene.overlaps`` (default: those)."""

    def __init__(self, As: Dict[Hashable, np.ndarray], bs: Dict[Hashable, np.ndarray], n: int, device: int = 0, scene=None, pair_lp=None):
        from .scene import DeviceScene, PolytopeScene, build_graph_arrays_device
        if 's' in As or 't' in As:
            raise ValueError("SceneQueries takes the regions alone: the keys 's' and 't' belong to the queries")
        self.n, self.device = int(n), int(device)
        self.keys = list(As.keys())
        self.polys = [(np.asarray(As[k], float).reshape(-1, self.n), np.asarray(bs[k], float).ravel()) for k in self.keys]
        self._pair_lp = pair_lp or (lambda polys, pa, pb, tol, cen: PolytopeScene(polys, self.device).overlaps(pa, pb, tol, cen))
        self.scene = scene if scene is not None else DeviceScene(self.polys, self.device)
        try:
            self.stats = {}
            self._pairs = {}      # the decided pair list with the host's decisions in it: pa, pb, flags, status
            self.edge_tail, self.edge_head, self.centers = build_graph_arrays_device(
                self.polys, self.device, scene=self.scene, stats=self.stats, names=self.keys, broad_phase="device", pairs_out=self._pairs)
        except Exception:
            self.close()
            raise
        self.centers = np.ascontiguousarray(self.centers, float)
        self.last = {}      # counts of the last regions_at call: hits, undecided, redone_on_host
        # assemble="device" alone: is the scene's region graph that of _pairs?  The regions' stacked polytope CSR (rows int64, A, b)
        self._graph_resident, self._stacked = False, None

    def close(self):
        if getattr(self, "scene", None) is not None:
            self.scene.close()
            self.scene = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------
    def _take_pairs(self, pa, pb, flags, status, edit):
        from .scene import edge_arrays
        self._pairs = dict(pa=pa, pb=pb, flags=flags, status=status)
        self.edge_tail, self.edge_head = edge_arrays(pa, pb, flags)
        self._graph_resident = False
        self.stats.update(candidate_pairs=int(len(pa)), overlaps_redone_on_host=int((status < 0).sum()), **edit)

    def add_regions(self, As: Dict[Hashable, np.ndarray], bs: Dict[Hashable, np.ndarray], tol: float = 1e-9):
        """Add the regions ``As``, ``bs`` (new keys, in the dictionary's order, behind the old ones) without rebuilding the graph: the
        scene runs the LPs of the new regions and of the pairs they form (``DeviceScene.add_regions``), and the object is afterwards
        what a new ``SceneQueries`` on the joined dictionaries is.  The rules of construction hold: a centre LP with status < 0 raises
        GcsAdmmError and a radius <= 0 ValueError, both naming the keys and leaving the object as it was; a new pair whose LP reports
        status < 0 is decided by ``graph.polytopes_overlap``.  Pairs that were there keep their decision, the host's included.
        ``stats`` receives the LPs this edit ran: ``edit_centre_lps``, ``edit_bound_lps``, ``edit_pair_lps``."""
        from .abi import GcsAdmmError
        from .scene import check_centres
        if self.scene is None:
            raise RuntimeError("the scene is closed")
        new_keys = list(As.keys())
        if 's' in As or 't' in As:
            raise ValueError("SceneQueries takes the regions alone: the keys 's' and 't' belong to the queries")
        known = set(self.keys)
        twice = [k for k in new_keys if k in known]
        if twice:
            raise ValueError(f"regions {twice[:5]} are in the scene already")
        polys = [(np.asarray(As[k], float).reshape(-1, self.n), np.asarray(bs[k], float).ravel()) for k in new_keys]
        P_old = len(self.keys)
        try:
            cen, _, _, counts = self.scene.add_regions(polys, tol=tol)
        except GcsAdmmError as e:
            if getattr(e, "results", None) is not None:      # name the regions as construction does
                check_centres(e.results[1], e.results[2], lambda idx: [new_keys[i] for i in idx])
            raise
        pa, pb, flags, status = self.scene.pairs()
        new = pb >= P_old
        old = self._pairs
        if not (np.array_equal(pa[~new], old["pa"]) and np.array_equal(pb[~new], old["pb"])):
            raise RuntimeError("the scene's pair list lost its order")
        flags = np.array(flags, copy=True)
        flags[~new] = old["flags"]
        for t in np.nonzero(new & (status < 0))[0]:
            (A1, b1), (A2, b2) = (self.polys + polys)[pa[t]], (self.polys + polys)[pb[t]]
            flags[t] = 1 if polytopes_overlap(A1, b1, A2, b2) else 0
        self.keys = self.keys + new_keys
        self.polys = self.polys + polys
        if self._stacked is not None:      # extended by the new rows
            rows, A, b = self._stacked
            self._stacked = (np.concatenate([rows, rows[-1] + np.cumsum([len(q) for _, q in polys], dtype=np.int64)]),
                             np.concatenate([A] + [p for p, _ in polys]), np.concatenate([b] + [q for _, q in polys]))
        self.centers = np.ascontiguousarray(np.vstack([self.centers, np.asarray(cen, float).reshape(-1, self.n)]))
        self._take_pairs(pa, pb, flags, status, dict(edit_centre_lps=len(polys), edit_bound_lps=2 * self.n * len(polys),
                                                     edit_pair_lps=int(counts["new_pairs"])))

    def remove_regions(self, keys):
        """Take the regions ``keys`` out (``DeviceScene.remove_regions``): no LP runs, and the object is afterwards what a new
        ``SceneQueries`` on the remaining dictionaries is.  An unknown key or one given twice raises ValueError before any device call."""
        if self.scene is None:
            raise RuntimeError("the scene is closed")
        keys = list(keys)
        where = {k: i for i, k in enumerate(self.keys)}
        unknown = [k for k in keys if k not in where]
        if unknown or len(set(keys)) != len(keys):
            raise ValueError(f"regions {unknown[:5]} are not in the scene" if unknown else "a region is given twice")
        gone = np.array([where[k] for k in keys], np.int64)
        self.scene.remove_regions(gone)
        stays = np.ones(len(self.keys), bool)
        stays[gone] = False
        newidx = np.cumsum(stays) - 1
        old = self._pairs
        keep = stays[old["pa"]] & stays[old["pb"]]
        pa, pb, _, status = self.scene.pairs()
        if not (np.array_equal(pa, newidx[old["pa"][keep]]) and np.array_equal(pb, newidx[old["pb"][keep]])):
            raise RuntimeError("the scene's pair list lost its order")
        self.keys = [k for k, s in zip(self.keys, stays) if s]
        self.polys = [p for p, s in zip(self.polys, stays) if s]
        if self._stacked is not None:      # compacted: the rows of the regions that stay
            rows, A, b = self._stacked
            keep_rows = np.repeat(stays, np.diff(rows))
            self._stacked = (np.concatenate([[0], np.cumsum(np.diff(rows)[stays])]).astype(np.int64), A[keep_rows], b[keep_rows])
        self.centers = np.ascontiguousarray(self.centers[stays])
        self._take_pairs(pa, pb, old["flags"][keep], status, dict(edit_centre_lps=0, edit_bound_lps=0, edit_pair_lps=0))

    def regions_at(self, points, eps: float = 1e-6, tol: float = 1e-9):
        """The regions that meet the box ``[p - eps, p + eps]`` of each point, by the rule ``build_graph`` connects a terminal with: one
        ascending int32 array of region indices per point.  One ``locate`` call for all points; its UNDECIDED hits, all of them, go
        through ONE call of the pair LPs on a temporary scene of the point boxes and the distinct regions involved -- the point box first
        in every pair, its LP started at p; an LP that reports status < 0 is decided by ``graph.polytopes_overlap``."""
        if self.scene is None:
            raise RuntimeError("the scene is closed")
        pts = np.ascontiguousarray(points, float).reshape(-1, self.n)
        Q = pts.shape[0]
        hit_ptr, hit_region, hit_class = self.scene.locate(pts, eps, tol)
        keep = hit_class == IN
        und = np.nonzero(hit_class == UNDECIDED)[0]
        redone = 0
        if len(und):
            point_of = np.repeat(np.arange(Q), np.diff(hit_ptr))[und]
            qs, pa = np.unique(point_of, return_inverse=True)
            rs, pb = np.unique(hit_region[und], return_inverse=True)
            polys = [convert_pt_to_polytope(pts[q], eps) for q in qs] + [self.polys[r] for r in rs]
            start = np.vstack([pts[qs], self.centers[rs]])
            flags, status = self._pair_lp(polys, pa.astype(np.int32), (len(qs) + pb).astype(np.int32), tol, start)
            flags = np.array(flags, copy=True)
            for t in np.nonzero(np.asarray(status) < 0)[0]:
                flags[t] = 1 if polytopes_overlap(*polys[pa[t]], *polys[len(qs) + pb[t]]) else 0
                redone += 1
            keep[und] = flags != 0
        self.last = dict(hits=int(len(hit_region)), undecided=int(len(und)), redone_on_host=redone)
        counts = np.bincount(np.repeat(np.arange(Q), np.diff(hit_ptr))[keep], minlength=Q)
        return np.split(hit_region[keep].astype(np.int32), np.cumsum(counts)[:-1]) if Q else []

    def _assemble_on_device(self, S, G, regs, eps):
        """the graphs of ``graphs`` from ONE ``query_graphs`` call: the scene's region graph (built on first use and after an edit, with
        the host's decisions in it when an LP left a pair undecided) merged with every query's terminal edges by a kernel, the arrays
        taken as they come; the polytope CSR is the regions' stacked one behind the two point boxes"""
        B = len(S)
        if not self._graph_resident:
            undecided = np.any(np.asarray(self._pairs["status"]) < 0)
            self.scene.build_region_graph(self._pairs["flags"] if undecided else None)
            self._graph_resident = True
        if self._stacked is None:
            rows = np.zeros(len(self.polys) + 1, np.int64)
            rows[1:] = np.cumsum([len(b) for _, b in self.polys])
            self._stacked = (rows, np.ascontiguousarray(np.vstack([A for A, _ in self.polys]).reshape(-1, self.n)) if self.polys else np.zeros((0, self.n)),
                             np.ascontiguousarray(np.hstack([b for _, b in self.polys])) if self.polys else np.zeros(0))
        rows, A_all, b_all = self._stacked
        term_ptr = np.zeros(2 * B + 1, np.int64)
        term_ptr[1:] = np.cumsum([len(r) for r in regs])
        term_region = np.concatenate(regs) if regs else np.zeros(0, np.int32)
        st = np.array([np.all(np.maximum(S[i] - eps, G[i] - eps) <= np.minimum(S[i] + eps, G[i] + eps) + 1e-9) for i in range(B)], np.uint8)
        arrays = self.scene.query_graphs(term_ptr, term_region, st)
        keys = ['s', 't'] + self.keys
        poly_ptr = np.concatenate([[0, 2 * self.n, 4 * self.n], rows[1:] + 4 * self.n]).astype(np.int32)
        out = []
        for i in range(B):
            (A_s, b_s), (A_t, b_t) = convert_pt_to_polytope(S[i], eps), convert_pt_to_polytope(G[i], eps)
            tail, head, inc_ptr, inc_edge, inc_out, inc_tail, inc_head = arrays[i]
            out.append(GcsGraph(n=self.n, keys=list(keys), edge_tail=tail, edge_head=head, inc_ptr=inc_ptr, inc_edge=inc_edge, inc_out=inc_out,
                                edge_inc_tail=inc_tail, edge_inc_head=inc_head, poly_ptr=poly_ptr.copy(),
                                poly_A=np.concatenate([np.asarray(A_s, float).reshape(-1, self.n), np.asarray(A_t, float).reshape(-1, self.n), A_all]),
                                poly_b=np.concatenate([np.asarray(b_s, float).ravel(), np.asarray(b_t, float).ravel(), b_all]),
                                interior=np.concatenate([S[i][None], G[i][None], self.centers]), src=0, dst=1))
        return out

    def graphs(self, starts, goals, eps: float = 1e-6, tol: float = 1e-9, assemble: str = "host"):
        """One ``GcsGraph`` per query ``(starts[i], goals[i])``, keys ``['s', 't', *region keys]``: what ``graph_from_sets`` makes of the
        sets ``{'s': box of the start, 't': box of the goal, regions}`` -- the region edges shifted by two, both directions of every
        terminal-region hit, and both directions of s-t when the two boxes meet (the interval rule of ``graph.polytopes_overlap``), in
        double-loop order.  ``interior`` is the point itself for a terminal and the scene's centre for a region.  A start or goal whose
        box meets no region raises ValueError.

        ``assemble``: ``"host"`` (the default: one ``lexsort`` over all edges and ``graph._finish_graph`` per query) or ``"device"`` (the
        region graph is built once on the scene, where the pair list lives, and ONE kernel call writes the index arrays of all queries
        -- csrc/query_graph_core.h --; every field of every graph is the host path's, dtype, shape and bytes)."""
        if assemble not in ("host", "device"):
            raise ValueError(f"assemble must be 'host' or 'device', not {assemble!r}")
        S = np.ascontiguousarray(starts, float).reshape(-1, self.n)
        G = np.ascontiguousarray(goals, float).reshape(-1, self.n)
        if len(S) != len(G):
            raise ValueError("one goal for every start")
        B = len(S)
        regs = self.regions_at(np.vstack([S, G]), eps, tol)
        for i in range(B):
            for which, r in (("start", regs[i]), ("goal", regs[B + i])):
                if len(r) == 0:
                    raise ValueError(f"query {i}: the {which} lies in no region")
        if assemble == "device":
            return self._assemble_on_device(S, G, regs, eps)
        box = lambda p: (p - eps, p + eps)      # the bounds graph._as_box reads off convert_pt_to_polytope(p, eps)
        keys = ['s', 't'] + self.keys
        out = []
        for i in range(B):
            rs, rt = regs[i].astype(np.int64) + 2, regs[B + i].astype(np.int64) + 2
            (lo_s, hi_s), (lo_t, hi_t) = box(S[i]), box(G[i])
            st = np.array([0], np.int64) if np.all(np.maximum(lo_s, lo_t) <= np.minimum(hi_s, hi_t) + 1e-9) else np.zeros(0, np.int64)
            zs, zt = np.zeros(len(rs), np.int64), np.ones(len(rt), np.int64)
            tail = np.concatenate([self.edge_tail.astype(np.int64) + 2, zs, rs, zt, rt, st, st + 1])
            head = np.concatenate([self.edge_head.astype(np.int64) + 2, rs, zs, rt, zt, st + 1, st])
            o = np.lexsort((head, tail))
            polys = [convert_pt_to_polytope(S[i], eps), convert_pt_to_polytope(G[i], eps)] + self.polys
            out.append(_finish_graph(self.n, keys, tail[o], head[o], polys, np.vstack([S[i], G[i], self.centers]), 0, 1))
        return out

    def solve(self, starts, goals, state_dtype: str = "f64", N: int = 5, M: int = 20, seeds=None, params=None, return_state: bool = False,
              walk: str = "host", assemble: str = "host", **common):
        """Every query to its stop test in one ``BatchSolver`` (``params``: one dict per query, ``common``: parameters of all, as
        ``BatchSolver.solve``), then rounded by ``rounding_many`` (``N``, ``M``: as ``rounding``; ``seeds``: one per query, default 0).
        ``walk``: ``"host"`` (the default: the walks of ``rounding``, on a host copy of every query's activations) or ``"device"``
        (``rounding_members``: the walks of all queries drawn on the device while the activations are still there, by the rule of
        ``walks.walk_reference`` -- other draws than the host's for the same seed).  ``assemble``: as ``graphs`` (the same graphs either way).
        Returns one record per query: that of ``DeviceSolver.solve`` plus ``rounded_cost``, ``x_v_rounded``, ``y_v_rounded`` and
        ``graph``; with ``return_state`` also ``trace`` and ``state``, host copies of the member's trace and of its six state arrays (the
        batch and its members are closed on return)."""
        from .batch import BatchSolver
        from .graph import sets_of_graph
        from .rounding import rounding_many, rounding_members, rounding_problem
        if walk not in ("host", "device"):
            raise ValueError(f"walk must be 'host' or 'device', not {walk!r}")
        graphs = self.graphs(starts, goals, assemble=assemble)
        seeds = [0] * len(graphs) if seeds is None else list(seeds)
        if len(seeds) != len(graphs):
            raise ValueError("one seed per query")
        batch = BatchSolver(graphs, state_dtype, device=self.device)

        def close():
            batch.close()
            for m in batch.members:
                m.close()

        def keep(records):
            for rec, m, g in zip(records, batch.members, graphs):
                rec["graph"] = g
                if return_state:
                    rec["trace"] = m.trace.cpu().numpy()
                    rec["state"] = {k: getattr(m, k).cpu().numpy() for k in ("copy", "mu", "zedge", "xv", "zv", "yv")}
        with contextlib.ExitStack() as members_open:
            members_open.callback(close)
            records = batch.solve(params=params, **common)
            if walk == "device":         # the walks read the activations where the members hold them
                rounded = rounding_members(batch.members, graphs, N=N, M=M, seeds=seeds, device=self.device)
                keep(records)
            else:                        # the host walks read a copy of them; the batch is closed before the rounding
                problems = [rounding_problem(m, *sets_of_graph(g), seed=s) for m, g, s in zip(batch.members, graphs, seeds)]
                keep(records)
                members_open.close()
                rounded = rounding_many(problems, N=N, M=M, device=self.device)
        for rec, (cost, x_v, y_v) in zip(records, rounded):
            rec.update(rounded_cost=cost, x_v_rounded=x_v, y_v_rounded=y_v)
        return records
