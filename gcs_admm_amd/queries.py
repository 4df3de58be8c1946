"""Many start / goal queries on one scene: the use case ``batch.py`` names for ``BatchSolver``.

A query differs from the next one only in its two terminals, so the region graph -- the centre LPs, the box LPs, the sweep and every
region-region overlap LP -- is decided ONCE, on a resident ``DeviceScene``.  Per call, ``locate_kernel`` (csrc/point_locate_core.h)
lists the regions under every start and goal point; only hits in the band of about 1e-6 around a facet or a vertex go to a pair LP,
all of them in one call.  The query graphs are the region graph plus the terminals' edges, in the order and with the arrays a
from-scratch ``graph_from_sets_device`` on ``{'s', 't', regions}`` gives; ``solve`` takes them through ``BatchSolver`` and
``rounding_many``.  By default the graphs are assembled on the host (a sort over all edges per query); ``assemble="device"`` takes them
from one kernel call on the scene's own region graph (csrc/query_graph_core.h), the same arrays.  ``prune="informed"`` runs every query on
its informed region set alone (``informed``, csrc/informed_core.h): the regions within the length of a feasible path of both terminals,
which loses no optimal path (``prune="informed_sets"``: the same between start and goal sets, csrc/informed_set_core.h); ``assemble="induced"`` builds those pruned graphs on the device too (csrc/induced_graph_core.h), in work
proportional to the kept set.  The scene is not frozen: ``add_regions`` and ``remove_regions`` edit it in place, and only the LPs of what is new run.  There is no CPU fallback: the LPs and the locate call run on the device (tests inject stand-ins).
"""
from __future__ import annotations

import contextlib
from typing import Dict, Hashable

import numpy as np

from .graph import GcsGraph, _finish_graph, convert_pt_to_polytope, polytopes_overlap

__all__ = ["SceneQueries", "rounded_path", "rounded_polyline"]

IN, UNDECIDED = 1, 2      # hit classes of gcsadmm_scene_locate_points


def rounded_path(record):
    """The vertex keys of the rounded path of a ``SceneQueries.solve`` record, from ``'s'`` to ``'t'``.  A vertex of the rounded path
    holds one segment of it (``x_v_rounded[v]``: its two end points); the walk goes over the record's graph along the vertices with
    ``y_v_rounded == 1``, at each step to the successor whose first point is the current vertex's second point.  ValueError: the
    record has no rounded path."""
    g, xs, ys = record["graph"], record.get("x_v_rounded"), record.get("y_v_rounded")
    if xs is None or ys is None:
        raise ValueError("the record has no rounded path")
    n, keys = g.n, g.keys
    cur = keys[g.src]
    if not ys.get(cur) or not ys.get(keys[g.dst]):
        raise ValueError("the record has no rounded path")
    path = [cur]
    while cur != keys[g.dst]:
        heads = [keys[h] for h in g.edge_head[g.edge_tail == keys.index(cur)]]
        nxt = [w for w in heads if ys.get(w) and w not in path and np.array_equal(xs[w][:n], xs[cur][n:])]
        if not nxt:
            raise ValueError(f"the rounded path ends at {cur!r}")
        cur = nxt[0]
        path.append(cur)
    return path


def rounded_polyline(record):
    """The points q_0 .. q_k of the rounded path of a ``SceneQueries.solve`` record (``rounded_path``: the first point of ``'s'``, then
    the second point of every vertex), as ``SceneQueries.path_cover`` takes them.  Consecutive equal points are dropped."""
    xs, n = record["x_v_rounded"], record["graph"].n
    path = rounded_path(record)
    points = [np.asarray(xs[path[0]][:n], float)] + [np.asarray(xs[v][n:], float) for v in path]
    keep = [0] + [i for i in range(1, len(points)) if not np.array_equal(points[i], points[i - 1])]
    return np.array([points[i] for i in keep])


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
        # replanning: a serial number per region that survives every edit -- 0 .. P-1 now, the next free ones in add_regions, never
        # reused after remove_regions; a query graph's vertex ids are made of them (vertex_ids)
        self.serials, self._next_serial = list(range(len(self.keys))), len(self.keys)
        self.last = {}      # counts of the last regions_at call: hits, undecided, redone_on_host
        self.snapped = []   # per query of the last graphs / solve call: what outside="snap" replaced (_snap)
        # assemble="device" / "induced" and informed: is the scene's region graph that of _pairs?  The two assemblies: the regions' stacked
        # polytope CSR (rows int64, A, b)
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
        self.serials = self.serials + list(range(self._next_serial, self._next_serial + len(new_keys)))
        self._next_serial += len(new_keys)
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
        self.serials = [r for r, s in zip(self.serials, stays) if s]
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
        return self._decide(self.scene.locate(pts, eps, tol), pts, lambda q: convert_pt_to_polytope(pts[q], eps), tol)

    def regions_meeting(self, lo, hi, tol: float = 1e-9):
        """``regions_at`` for boxes: the regions that meet each box ``[lo[q], hi[q]]`` ([Q, n] each), one ascending int32 array of region
        indices per box.  One ``locate_boxes`` call (csrc/box_locate_core.h) for all boxes; its UNDECIDED hits -- for a box as wide as a
        region, every region that reaches into it without holding its centre -- go through ONE call of the pair LPs, the box as the
        polytope ``[I; -I] x <= [hi; -lo]`` first in every pair, its LP started at the box's centre; an LP that reports status < 0 is
        decided by ``graph.polytopes_overlap``.  ``last`` is filled as ``regions_at`` fills it."""
        if self.scene is None:
            raise RuntimeError("the scene is closed")
        lo = np.ascontiguousarray(lo, float).reshape(-1, self.n); hi = np.ascontiguousarray(hi, float).reshape(-1, self.n)
        if lo.shape != hi.shape:
            raise ValueError("lo and hi must have one shape")
        return self._decide(self.scene.locate_boxes(lo, hi, tol), 0.5 * (lo + hi), lambda q: self._box_polytope(lo[q], hi[q]), tol)

    def _box_polytope(self, lo, hi):
        """the box as ``graph_from_sets`` is given it: ``[I; -I] x <= [hi; -lo]``"""
        return np.vstack([np.eye(self.n), -np.eye(self.n)]), np.hstack([np.asarray(hi, float), -np.asarray(lo, float)])

    def _decide(self, hits, pts, term_poly, tol):
        """the region lists of a hit list: the IN hits and those UNDECIDED hits that one call of the pair LPs (terminal ``term_poly(q)``
        first, started at ``pts[q]``) or, after a status < 0, ``graph.polytopes_overlap`` finds to overlap"""
        hit_ptr, hit_region, hit_class = hits
        Q = pts.shape[0]
        keep = hit_class == IN
        und = np.nonzero(hit_class == UNDECIDED)[0]
        redone = 0
        if len(und):
            point_of = np.repeat(np.arange(Q), np.diff(hit_ptr))[und]
            qs, pa = np.unique(point_of, return_inverse=True)
            rs, pb = np.unique(hit_region[und], return_inverse=True)
            polys = [term_poly(q) for q in qs] + [self.polys[r] for r in rs]
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

    def nearest_regions(self, points, radius=None):
        """For points that may lie in NO region: per point ``(region index, distance, projected point)`` of the nearest region -- the
        Euclidean projection of the point onto it, the point itself at distance 0 when it lies in a region -- or ``(-1, inf, None)``
        when no region is within ``radius`` of it.  One ``project`` call for all points (csrc/point_project_core.h).  ``radius``: one
        value or one per point; default per point ``min_r |p - c_r|`` over the resident Chebyshev centres -- a centre lies in its
        region, so the nearest region is always within it.  The nearest region is the solved hit within the radius of least distance,
        the lowest region index among equals.  A pair whose solve failed on the device (status -1) is solved again on the host by
        ``scipy.optimize.minimize(method="SLSQP")`` from the region's centre; ``last`` counts them (``redone_on_host``)."""
        if self.scene is None:
            raise RuntimeError("the scene is closed")
        pts = np.ascontiguousarray(points, float).reshape(-1, self.n)
        Q = pts.shape[0]
        if radius is None:
            rad = np.array([np.sqrt(((self.centers - p) ** 2).sum(axis=1)).min() for p in pts]) if len(self.keys) else np.full(Q, np.inf)
        else:
            rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, float), (Q,)))
        hit_ptr, hit_region, _, distance, nearest, status, _ = self.scene.project(pts, rad)
        distance, nearest, status = np.array(distance, float), np.array(nearest, float).reshape(-1, self.n), np.array(status, np.int32)
        point_of = np.repeat(np.arange(Q), np.diff(hit_ptr))
        failed = np.nonzero(status < 0)[0]
        for t in failed:
            p = pts[point_of[t]]
            x = self._project_on_host(int(hit_region[t]), p)
            nearest[t], distance[t] = x, float(np.sqrt(((x - p) ** 2).sum()))
            status[t] = 0 if distance[t] <= rad[point_of[t]] else 1
        self.last = dict(hits=int(len(hit_region)), undecided=int(len(failed)), redone_on_host=int(len(failed)))
        out = []
        for q in range(Q):
            seg = np.arange(hit_ptr[q], hit_ptr[q + 1])
            seg = seg[status[seg] == 0]
            if len(seg) == 0:
                out.append((-1, np.inf, None))
                continue
            t = seg[np.argmin(distance[seg])]      # (region indices ascend: the first of equals is the lowest)
            out.append((int(hit_region[t]), float(distance[t]), nearest[t].copy()))
        return out

    def path_cover(self, paths, tol: float = 1e-9):
        """Is each of ``paths`` -- polylines ``[k + 1, n]`` -- inside the union of the resident regions, and through which regions does it
        run?  All segments of all paths go into one ``clip_segments`` call (csrc/segment_clip_core.h: per segment the spans of the
        regions it meets, inflated by ``tol``, and the shortest chain of them that covers it).  Per path a dict: ``covered``; ``gap``:
        None, or for the first segment that is not covered ``dict(segment=j, t=reach, point=p + reach d)``, the first parameter no region
        holds; ``corridor``: the region keys of the chains of its segments in order, consecutive repeats merged (the form
        ``DeviceScene.restrict_paths`` takes); ``breaks``: the points ``x(t_out)`` at which the corridor passes from one region to the
        next; ``adjacent``: whether every consecutive pair of the corridor is an edge of the resident region graph -- informative: two
        regions that touch only within the inflation can share a break without being an edge."""
        if self.scene is None:
            raise RuntimeError("the scene is closed")
        lines = [np.ascontiguousarray(p, float).reshape(-1, self.n) for p in paths]
        if any(len(p) < 2 for p in lines):
            raise ValueError("a polyline has at least two points")
        start = np.concatenate([p[:-1] for p in lines]) if lines else np.zeros((0, self.n))
        end = np.concatenate([p[1:] for p in lines]) if lines else np.zeros((0, self.n))
        _, hit_region, _, _, t_out, status, reach, chain_ptr, chain_hit = self.scene.clip_segments(start, end, tol)
        edges = set(zip(np.asarray(self.edge_tail).tolist(), np.asarray(self.edge_head).tolist()))
        out, q = [], 0
        for line in lines:
            corridor, breaks, gap, last = [], [], None, None
            for j in range(len(line) - 1):
                d = end[q] - start[q]
                for c in chain_hit[chain_ptr[q]:chain_ptr[q + 1]]:
                    r = int(hit_region[c])
                    if not corridor or corridor[-1] != r:
                        if corridor:
                            breaks.append(last)
                        corridor.append(r)
                    last = start[q] + t_out[c] * d
                if status[q] != 0 and gap is None:
                    gap = dict(segment=j, t=float(reach[q]), point=start[q] + reach[q] * d)
                q += 1
            out.append(dict(covered=gap is None, gap=gap, corridor=[self.keys[r] for r in corridor], breaks=breaks,
                            adjacent=all((a, b) in edges or (b, a) in edges for a, b in zip(corridor, corridor[1:]))))
        return out

    def _project_on_host(self, r, p):
        """the projection of p onto region r by SLSQP, started at the region's centre: what a failed device solve falls back to"""
        from scipy.optimize import minimize
        A, b = self.polys[r]
        res = minimize(lambda x: 0.5 * float((x - p) @ (x - p)), self.centers[r], jac=lambda x: x - p, method="SLSQP",
                       constraints=[dict(type="ineq", fun=lambda x: b - A @ x, jac=lambda x: -A)], options=dict(ftol=1e-15, maxiter=200))
        return np.asarray(res.x, float)

    def _snap(self, S, G, regs, eps, tol, snap_radius, sb=None, gb=None):
        """``outside="snap"``: every point terminal that lies in no region is replaced, in S / G and in ``regs``, by its projection onto
        its nearest region -- one ``project`` call for all of them, one more ``regions_at`` call for the replaced points alone.  Returns
        the ``snapped`` records, one dict(start=, goal=) per query"""
        B = len(S)
        snapped = [dict(start=None, goal=None) for _ in range(B)]
        out = [(which, i) for i in range(B) for which, r, boxes in (("start", regs[i], sb), ("goal", regs[B + i], gb)) if len(r) == 0 and boxes is None]
        if not out:
            return snapped
        side = lambda which: S if which == "start" else G
        counts = dict(self.last)
        found = self.nearest_regions(np.array([side(which)[i] for which, i in out]), snap_radius)
        counts = {k: v + self.last[k] for k, v in counts.items()}
        for (which, i), (r, d, x) in zip(out, found):
            if r < 0:
                raise ValueError(f"query {i}: the {which} lies in no region"
                                 + ("" if snap_radius is None else f", and no region is within {np.ravel(snap_radius)[0]:g} of it"))
            snapped[i][which] = dict(original=side(which)[i].copy(), point=x, region=self.keys[r], distance=d)
        again = self.regions_at(np.array([x for _, _, x in found]), eps, tol)
        self.last = {k: v + self.last[k] for k, v in counts.items()}
        for (which, i), (r, _, x), lst in zip(out, found, again):
            if r not in lst.tolist():
                raise RuntimeError(f"query {i}: the projected {which} is not found in its nearest region {self.keys[r]!r}")
            side(which)[i] = x
            regs[i if which == "start" else B + i] = lst
        return snapped

    def _region_graph_on_device(self):
        """the scene's region graph is that of ``_pairs``: built on first use and after an edit, with the host's decisions in it when an
        LP left a pair undecided"""
        if not self._graph_resident:
            undecided = np.any(np.asarray(self._pairs["status"]) < 0)
            self.scene.build_region_graph(self._pairs["flags"] if undecided else None)
            self._graph_resident = True

    @staticmethod
    def _term_lists(regs):
        term_ptr = np.zeros(len(regs) + 1, np.int64)
        term_ptr[1:] = np.cumsum([len(r) for r in regs])
        return term_ptr, (np.concatenate(regs) if regs else np.zeros(0, np.int32))

    MIN_HALF_WIDTH = 1e-5      # of a box terminal: above it gcsadmm_create takes the terminal for a region, and the box has an interior

    def _box_terminals(self, boxes, which):
        """(lo [B, n], hi [B, n]) of ``start_boxes`` / ``goal_boxes``; a box thinner than a region may be is refused"""
        lo, hi = boxes
        lo = np.ascontiguousarray(lo, float).reshape(-1, self.n); hi = np.ascontiguousarray(hi, float).reshape(-1, self.n)
        if lo.shape != hi.shape:
            raise ValueError(f"{which}_boxes: lo and hi must have one shape")
        if lo.size and not np.all(0.5 * (hi - lo) > self.MIN_HALF_WIDTH):
            raise ValueError(f"{which}_boxes: every half-width must exceed {self.MIN_HALF_WIDTH:g}: give a point as a point ({which}s)")
        return lo, hi

    def _located(self, starts, goals, eps, tol, start_boxes=None, goal_boxes=None, outside="raise", snap_radius=None):
        """(S [B, n], G [B, n], the region lists of ``regions_at`` / ``regions_meeting`` for the starts, then the goals, (lo, hi) of the
        start boxes or None, (lo, hi) of the goal boxes or None); S, G: the points, or the centres of the boxes.
        A terminal that meets no region raises -- with ``outside="snap"`` a point terminal is first replaced by its projection onto
        its nearest region (``_snap``); ``snapped`` has one record dict(start=, goal=) per query of what was replaced"""
        if outside not in ("raise", "snap"):
            raise ValueError(f"outside must be 'raise' or 'snap', not {outside!r}")
        for which, pts, boxes in (("start", starts, start_boxes), ("goal", goals, goal_boxes)):
            if (pts is None) == (boxes is None):
                raise ValueError(f"give exactly one of {which}s and {which}_boxes")
        sb = self._box_terminals(start_boxes, "start") if start_boxes is not None else None
        gb = self._box_terminals(goal_boxes, "goal") if goal_boxes is not None else None
        S = np.array(starts, float).reshape(-1, self.n) if sb is None else 0.5 * (sb[0] + sb[1])      # (copies: a snap writes into them)
        G = np.array(goals, float).reshape(-1, self.n) if gb is None else 0.5 * (gb[0] + gb[1])
        if len(S) != len(G):
            raise ValueError("one goal for every start")
        B = len(S)
        if sb is None and gb is None:
            regs = self.regions_at(np.vstack([S, G]), eps, tol)
        elif sb is not None and gb is not None:
            regs = self.regions_meeting(np.vstack([sb[0], gb[0]]), np.vstack([sb[1], gb[1]]), tol)
        else:      # a point on one side, a box on the other: one locate call each; `last` adds the two up
            first = self.regions_at(S, eps, tol) if sb is None else self.regions_meeting(*sb, tol)
            counts = dict(self.last)
            regs = first + (self.regions_at(G, eps, tol) if gb is None else self.regions_meeting(*gb, tol))
            self.last = {k: v + counts[k] for k, v in self.last.items()}
        self.snapped = self._snap(S, G, regs, eps, tol, snap_radius, sb, gb) if outside == "snap" else [dict(start=None, goal=None) for _ in range(B)]
        for i in range(B):
            for which, r in (("start", regs[i]), ("goal", regs[B + i])):
                if len(r) == 0:
                    raise ValueError(f"query {i}: the {which} lies in no region")
        return S, G, regs, sb, gb

    def informed(self, starts, goals, eps: float = 1e-6, tol: float = 1e-9, restrict=None):
        """The informed region set of every query (csrc/informed_core.h): the regions an optimal path can touch lie in the ellipsoid with
        foci start and goal whose major axis is the length of any feasible path.  Per query a dict: ``path`` (int32 region indices of a
        shortest path on the region graph under the distances between centres, one ``region_paths`` call for all queries; empty when
        there is none), ``bound`` (the cost of the convex restriction along ``('s', *path, 't')``, all of them in one ``restrict`` call on
        the terminal boxes and the distinct path regions; ``inf`` without a path or when the restriction is infeasible or failed),
        ``keep`` (bool [P], one ``informed_regions`` call: the regions whose padded box is within the bound of both terminals; all of
        them for an ``inf`` bound) and ``restriction`` (the points of the bound's path by vertex key, or None).  The terminals are boxes
        of half-width ``eps`` around the points the kernel measures from, so the kernel's bound is ``bound + 4 eps sqrt(n)``, and the
        regions under the two points are kept whatever it says: both only widen the set.

        ``restrict``: ``(As, bs, n, paths) -> [(cost, xs)]`` as ``solver`` in ``rounding`` (default: ``solve_path_restrictions_device``).
        The boxes are moved out by ``scene.SWEEP_PAD``.  The region graph is built on the scene on first use and after an edit."""
        S, G, regs, _, _ = self._located(starts, goals, eps, tol)
        return self._informed(S, G, regs, eps, restrict)

    def informed_sets(self, starts=None, goals=None, start_boxes=None, goal_boxes=None, eps: float = 1e-6, tol: float = 1e-9, restrict=None):
        """``informed`` for start and goal SETS (csrc/informed_set_core.h): exactly one of ``starts`` / ``start_boxes`` and of ``goals`` /
        ``goal_boxes``, as ``graphs`` takes them, in every mix.  The records are those of ``informed``.  The path comes from one
        ``region_paths_sets`` call and the flags from one ``informed_regions_sets`` call: a region is kept when the distances of its
        padded box to the start set and to the goal set add up to at most the bound, which loses no optimal path between a point of the
        one and a point of the other.  A point goes to the two calls as the box ``lo == hi == p`` and to the restriction as its box of
        half-width ``eps``, a box to both as itself; the kernel's bound is ``bound + 2 k eps sqrt(n)`` with k the number of point
        terminals of the query (a box is measured from the very set the restriction used).  The regions under both terminals are kept
        whatever the flags say.  On point queries the records equal ``informed``'s."""
        S, G, regs, sb, gb = self._located(starts, goals, eps, tol, start_boxes, goal_boxes)
        return self._informed(S, G, regs, eps, restrict, sets=True, sb=sb, gb=gb)

    def _informed(self, S, G, regs, eps, restrict=None, sets=False, sb=None, gb=None):
        """the records of ``informed``, or (``sets``; ``sb``, ``gb``: the (lo, hi) of a side given as boxes) of ``informed_sets``"""
        from .rounding import solve_path_restrictions_device
        B = len(S)
        if B == 0:
            return []
        restrict = restrict or (lambda As, bs, n, paths: solve_path_restrictions_device(As, bs, n, paths, self.device))
        self._region_graph_on_device()
        points = np.vstack([S, G])
        if sets:      # what the kernels measure from: the boxes, a point as the box lo == hi
            lo = np.vstack([S if sb is None else sb[0], G if gb is None else gb[0]])
            hi = np.vstack([S if sb is None else sb[1], G if gb is None else gb[1]])
            paths, _, status = self.scene.region_paths_sets(lo, hi, *self._term_lists(regs))
        else:
            paths, _, status = self.scene.region_paths(points, *self._term_lists(regs))
        As, bs, jobs, owner = {}, {}, [], []
        for i in range(B):
            if status[i] != 0:
                continue
            for key, p, box in ((('s', i), S[i], self._box_of(sb, i)), (('t', i), G[i], self._box_of(gb, i))):
                As[key], bs[key] = convert_pt_to_polytope(p, eps) if box is None else self._box_polytope(*box)
            for r in paths[i]:
                As[('r', int(r))], bs[('r', int(r))] = self.polys[r]
            jobs.append([('s', i)] + [('r', int(r)) for r in paths[i]] + [('t', i)])
            owner.append(i)
        bound, points_of = np.full(B, np.inf), [None] * B
        if jobs:
            name = lambda k: k[0] if k[0] in ('s', 't') else self.keys[k[1]]
            for i, (cost, xs) in zip(owner, restrict(As, bs, self.n, jobs)):
                if xs is not None and np.isfinite(cost):
                    bound[i], points_of[i] = float(cost), {name(k): x for k, x in xs.items()}
        if sets:      # (the set call takes finite bounds: a query without one keeps every region, here)
            finite = np.isfinite(bound)
            widened = bound + (2.0 * ((sb is None) + (gb is None))) * eps * np.sqrt(self.n)
            keep = self.scene.informed_regions_sets(lo, hi, np.where(finite, widened, 0.0))
        else:
            keep = self.scene.informed_regions(points, bound + 4.0 * eps * np.sqrt(self.n))
        keep = np.array(keep, dtype=bool, copy=True)
        if sets:
            keep[~finite] = True
        for i in range(B):
            keep[i, regs[i]] = True
            keep[i, regs[B + i]] = True
        return [dict(path=np.asarray(paths[i], np.int32), bound=float(bound[i]), keep=keep[i], restriction=points_of[i]) for i in range(B)]

    def _host_graph(self, s, g, rs, rt, eps, keep=None, sbox=None, gbox=None):
        """the graph of one query from one ``lexsort`` over all edges and ``graph._finish_graph``: on all regions, or (``keep``: bool [P]) on
        the induced subgraph of the kept ones, renumbered in scene order.  ``sbox``, ``gbox``: (lo, hi) of a terminal that is a box (s, g
        are then its centre)"""
        tail_r, head_r, keys, polys, centers = self.edge_tail, self.edge_head, self.keys, self.polys, self.centers
        if keep is not None:
            idx = np.nonzero(keep)[0]
            new = np.cumsum(keep) - 1
            both = keep[tail_r] & keep[head_r]
            tail_r, head_r = new[tail_r[both]], new[head_r[both]]
            keys, polys, centers = [keys[r] for r in idx], [polys[r] for r in idx], centers[idx]
            rs, rt = new[rs], new[rt]
        rs, rt = rs.astype(np.int64) + 2, rt.astype(np.int64) + 2
        # the bounds graph._as_box reads off convert_pt_to_polytope(p, eps), or off the box itself
        (lo_s, hi_s), (lo_t, hi_t) = sbox or (s - eps, s + eps), gbox or (g - eps, g + eps)
        st = np.array([0], np.int64) if np.all(np.maximum(lo_s, lo_t) <= np.minimum(hi_s, hi_t) + 1e-9) else np.zeros(0, np.int64)
        zs, zt = np.zeros(len(rs), np.int64), np.ones(len(rt), np.int64)
        tail = np.concatenate([tail_r.astype(np.int64) + 2, zs, rs, zt, rt, st, st + 1])
        head = np.concatenate([head_r.astype(np.int64) + 2, rs, zs, rt, zt, st + 1, st])
        o = np.lexsort((head, tail))
        polys = [self._box_polytope(*sbox) if sbox else convert_pt_to_polytope(s, eps),
                 self._box_polytope(*gbox) if gbox else convert_pt_to_polytope(g, eps)] + polys
        return _finish_graph(self.n, ['s', 't'] + keys, tail[o], head[o], polys, np.vstack([s, g, centers]), 0, 1)

    def _stack(self):
        """the regions' stacked polytope CSR (rows int64, A, b): made on first use, kept across edits"""
        if self._stacked is None:
            rows = np.zeros(len(self.polys) + 1, np.int64)
            rows[1:] = np.cumsum([len(b) for _, b in self.polys])
            self._stacked = (rows, np.ascontiguousarray(np.vstack([A for A, _ in self.polys]).reshape(-1, self.n)) if self.polys else np.zeros((0, self.n)),
                             np.ascontiguousarray(np.hstack([b for _, b in self.polys])) if self.polys else np.zeros(0))
        return self._stacked

    @staticmethod
    def _box_of(boxes, i):
        """(lo, hi) of terminal i of ``boxes`` = (lo [B, n], hi [B, n]), or None for a side given as points"""
        return None if boxes is None else (boxes[0][i], boxes[1][i])

    @staticmethod
    def _adjacent(S, G, eps, sb=None, gb=None):
        """uint8 [B]: do the boxes of start and goal meet (the interval rule of ``_host_graph``)"""
        lo_s, hi_s = (S - eps, S + eps) if sb is None else sb
        lo_t, hi_t = (G - eps, G + eps) if gb is None else gb
        return np.array([np.all(np.maximum(lo_s[i], lo_t[i]) <= np.minimum(hi_s[i], hi_t[i]) + 1e-9) for i in range(len(S))], np.uint8)

    def _point_rows(self, s, g, eps, sbox=None, gbox=None):
        """the polytope rows of the two terminals of a query, point boxes or (``sbox``, ``gbox``) boxes: (A [4 n, n], b [4 n])"""
        A_s, b_s = self._box_polytope(*sbox) if sbox else convert_pt_to_polytope(s, eps)
        A_t, b_t = self._box_polytope(*gbox) if gbox else convert_pt_to_polytope(g, eps)
        return (np.concatenate([np.asarray(A_s, float).reshape(-1, self.n), np.asarray(A_t, float).reshape(-1, self.n)]),
                np.concatenate([np.asarray(b_s, float).ravel(), np.asarray(b_t, float).ravel()]))

    def _assemble_induced(self, S, G, regs, eps, info, sb=None, gb=None):
        """the pruned graphs of ``graphs`` from ONE ``induced_query_graphs`` call on the keep flags of ``_informed``: the induced subgraph
        of every query's kept set is built on the device from the rows of its kept regions (csrc/induced_graph_core.h), the arrays taken
        as they come; per query the host reads the P flags, and gathers the kept regions' rows of the stacked polytope CSR"""
        B = len(S)
        self._region_graph_on_device()
        rows, A_all, b_all = self._stack()
        term_ptr, term_region = self._term_lists(regs)
        keep = np.array([r["keep"] for r in info], np.uint8).reshape(B, len(self.keys))
        arrays = self.scene.induced_query_graphs(keep, term_ptr, term_region, self._adjacent(S, G, eps, sb, gb))
        out = []
        for i in range(B):
            idx = np.nonzero(keep[i])[0]
            counts = rows[idx + 1] - rows[idx]
            ends = np.cumsum(counts)
            take = np.repeat(rows[idx] - (ends - counts), counts) + np.arange(int(ends[-1]) if len(ends) else 0)      # the kept regions' rows
            A_pts, b_pts = self._point_rows(S[i], G[i], eps, self._box_of(sb, i), self._box_of(gb, i))
            tail, head, inc_ptr, inc_edge, inc_out, inc_tail, inc_head = arrays[i]
            out.append(GcsGraph(n=self.n, keys=['s', 't'] + [self.keys[r] for r in idx], edge_tail=tail, edge_head=head, inc_ptr=inc_ptr,
                                inc_edge=inc_edge, inc_out=inc_out, edge_inc_tail=inc_tail, edge_inc_head=inc_head,
                                poly_ptr=np.concatenate([[0, 2 * self.n, 4 * self.n], ends + 4 * self.n]).astype(np.int32),
                                poly_A=np.concatenate([A_pts, A_all[take]]), poly_b=np.concatenate([b_pts, b_all[take]]),
                                interior=np.concatenate([S[i][None], G[i][None], self.centers[idx]]), src=0, dst=1))
        return out

    def _assemble_on_device(self, S, G, regs, eps, sb=None, gb=None):
        """the graphs of ``graphs`` from ONE ``query_graphs`` call: the scene's region graph (built on first use and after an edit, with
        the host's decisions in it when an LP left a pair undecided) merged with every query's terminal edges by a kernel, the arrays
        taken as they come; the polytope CSR is the regions' stacked one behind the two point boxes"""
        B = len(S)
        self._region_graph_on_device()
        rows, A_all, b_all = self._stack()
        term_ptr, term_region = self._term_lists(regs)
        arrays = self.scene.query_graphs(term_ptr, term_region, self._adjacent(S, G, eps, sb, gb))
        keys = ['s', 't'] + self.keys
        poly_ptr = np.concatenate([[0, 2 * self.n, 4 * self.n], rows[1:] + 4 * self.n]).astype(np.int32)
        out = []
        for i in range(B):
            A_pts, b_pts = self._point_rows(S[i], G[i], eps, self._box_of(sb, i), self._box_of(gb, i))
            tail, head, inc_ptr, inc_edge, inc_out, inc_tail, inc_head = arrays[i]
            out.append(GcsGraph(n=self.n, keys=list(keys), edge_tail=tail, edge_head=head, inc_ptr=inc_ptr, inc_edge=inc_edge, inc_out=inc_out,
                                edge_inc_tail=inc_tail, edge_inc_head=inc_head, poly_ptr=poly_ptr.copy(),
                                poly_A=np.concatenate([A_pts, A_all]), poly_b=np.concatenate([b_pts, b_all]),
                                interior=np.concatenate([S[i][None], G[i][None], self.centers]), src=0, dst=1))
        return out

    def graphs(self, starts=None, goals=None, eps: float = 1e-6, tol: float = 1e-9, assemble: str = "host", prune=None, restrict=None,
               start_boxes=None, goal_boxes=None, outside: str = "raise", snap_radius=None):
        """One ``GcsGraph`` per query ``(starts[i], goals[i])``, keys ``['s', 't', *region keys]``: what ``graph_from_sets`` makes of the
        sets ``{'s': box of the start, 't': box of the goal, regions}`` -- the region edges shifted by two, both directions of every
        terminal-region hit, and both directions of s-t when the two boxes meet (the interval rule of ``graph.polytopes_overlap``), in
        double-loop order.  ``interior`` is the point itself for a terminal and the scene's centre for a region.  A start or goal whose
        box meets no region raises ValueError.

        ``start_boxes``, ``goal_boxes``: ``(lo [B, n], hi [B, n])``, a start or goal SET in the place of the point -- exactly one of
        ``starts`` / ``start_boxes`` is given, and likewise for the goals; a point start with a box goal is the common case.  Every
        half-width of a box must exceed 1e-5 (the box is then a region for ``gcsadmm_create`` and has an interior; a point is given as
        a point).  The terminal's polytope is ``[I; -I] x <= [hi; -lo]``, its ``interior`` the box's centre, its edges those of
        ``regions_meeting``, and s-t is decided by the interval rule on the two boxes: the graph is what ``graph_from_sets`` makes of
        ``{'s': box, 't': box, regions}``, field for field.  Such a graph has a terminal that is a region: ``solve`` runs it in a
        batch made with ``region_terminals``.  Not with ``prune="informed"``, whose bound is measured from points (csrc/informed_core.h);
        ``prune="informed_sets"`` measures from the sets.

        ``assemble``: ``"host"`` (the default: one ``lexsort`` over all edges and ``graph._finish_graph`` per query) or ``"device"`` (the
        region graph is built once on the scene, where the pair list lives, and ONE kernel call writes the index arrays of all queries
        -- csrc/query_graph_core.h --; every field of every graph is the host path's, dtype, shape and bytes).

        ``prune``: ``None`` (the default: every region) or ``"informed"``: the graph of query i is the host path's on the induced
        subgraph of its informed region set (``informed``; ``restrict`` as there), the regions renumbered in scene order, keys ``['s',
        't', *kept keys]``.  No optimal path is lost.  Not with ``assemble="device"``, which is the assembly of the WHOLE scene; the pruned
        one is ``assemble="induced"`` (only with ``prune``): one ``induced_query_graphs`` call builds the induced subgraph of every query's
        kept set on the device, from the rows of its kept regions alone -- csrc/induced_graph_core.h --, where ``"host"`` masks and
        renumbers the whole region edge list per query; every field of every graph is the host path's.  ``"informed_sets"``: the same
        with the set of ``informed_sets`` -- point or box terminals, in every mix, with ``assemble="host"`` or ``"induced"``.

        ``outside``: ``"raise"`` (the default: a terminal in no region raises) or ``"snap"``: a POINT terminal whose ``regions_at`` list
        is empty is replaced by its projection onto its nearest region (``nearest_regions``: all such points of the call in one
        ``project`` call, then ``regions_at`` again for the replaced points alone, whose list must hold the nearest region), and the
        graphs are those of the call with the replaced points, field for field: every later stage sees them and nothing else.
        ``snap_radius``: the farthest a point may be moved (default: as far as the nearest region is); a point with no region within
        it raises the ValueError.  Box terminals are untouched: a box that meets no region raises as before."""
        return self._graphs(starts, goals, eps, tol, assemble, prune, restrict, start_boxes, goal_boxes, outside, snap_radius)[0]

    def _graphs(self, starts, goals, eps, tol, assemble, prune, restrict, start_boxes=None, goal_boxes=None, outside="raise", snap_radius=None):
        """(the graphs of ``graphs``, the records of ``informed`` or None); ``snapped`` has the records of what ``outside="snap"`` replaced"""
        if assemble not in ("host", "device", "induced"):
            raise ValueError(f"assemble must be 'host' or 'device', or 'induced' with prune, not {assemble!r}")
        if prune not in (None, "informed", "informed_sets"):
            raise ValueError(f"prune must be None or 'informed' or 'informed_sets', not {prune!r}")
        if prune is not None and assemble == "device":
            raise ValueError("prune needs assemble='host' or 'induced': 'device' assembles the graphs of the whole scene")
        if prune is None and assemble == "induced":
            raise ValueError("assemble='induced' needs prune")
        if prune == "informed" and (start_boxes is not None or goal_boxes is not None):
            raise ValueError("prune='informed' takes point terminals: its bound is measured from the start and goal points "
                             "(prune='informed_sets' measures from sets)")
        S, G, regs, sb, gb = self._located(starts, goals, eps, tol, start_boxes, goal_boxes, outside, snap_radius)
        B = len(S)
        if assemble == "device":
            return self._assemble_on_device(S, G, regs, eps, sb, gb), None
        info = self._informed(S, G, regs, eps, restrict, sets=prune == "informed_sets", sb=sb, gb=gb) if prune else None
        if assemble == "induced":
            return (self._assemble_induced(S, G, regs, eps, info, sb, gb) if B else []), info
        return [self._host_graph(S[i], G[i], regs[i], regs[B + i], eps, info[i]["keep"] if prune else None, self._box_of(sb, i), self._box_of(gb, i))
                for i in range(B)], info

    def vertex_ids(self, graph):
        """The stable vertex ids of a query graph of this scene (``graphs``, or the ``graph`` of a ``solve`` record), int32: 0 for 's', 1
        for 't' and serial + 2 for a region, the serial being the number the region got when it entered the scene -- the same for
        every graph it appears in, pruned or not, before and after ``add_regions`` / ``remove_regions`` of others.  What
        ``StateSnapshot``s of this scene are keyed by.  Ids must ascend with the vertex index: a scene whose order of regions
        disagrees with their serials is refused, not sorted."""
        serial = dict(zip(self.keys, self.serials))
        try:
            ids = np.array([0, 1] + [serial[k] + 2 for k in graph.keys[2:]], np.int64)
        except KeyError as e:
            raise ValueError(f"region {e.args[0]!r} of the graph is not in the scene (any more)") from None
        if list(graph.keys[:2]) != ['s', 't'] or np.any(np.diff(ids) <= 0):
            raise RuntimeError("the order of the graph's regions and their serial numbers disagree: the vertex ids of a snapshot must "
                               "ascend with the vertex index")
        return ids.astype(np.int32)

    def solve(self, starts=None, goals=None, state_dtype: str = "f64", N: int = 5, M: int = 20, seeds=None, params=None, return_state: bool = False,
              walk: str = "host", assemble: str = "host", prune=None, restrict=None, large: bool = False, start_boxes=None, goal_boxes=None,
              keep: bool = False, seed=None, outside: str = "raise", snap_radius=None, **common):
        """Every query to its stop test in one ``BatchSolver`` (``params``: one dict per query, ``common``: parameters of all, as
        ``BatchSolver.solve``), then rounded by ``rounding_many`` (``N``, ``M``: as ``rounding``; ``seeds``: one per query, default 0).
        ``walk``: ``"host"`` (the default: the walks of ``rounding``, on a host copy of every query's activations) or ``"device"``
        (``rounding_members``: the walks of all queries drawn on the device while the activations are still there, by the rule of
        ``walks.walk_reference`` -- other draws than the host's for the same seed).  ``assemble``: as ``graphs`` (the same graphs whichever way; ``"induced"`` only with ``prune``).
        ``prune``, ``restrict``: as ``graphs``; with ``prune="informed"`` every query runs on its informed region set alone, each record
        gains ``informed_bound`` and ``kept_regions``, and the bound's path is one more candidate of the rounding step, so that
        ``rounded_cost <= informed_bound`` whenever the bound is finite; ``prune="informed_sets"`` does the same for box terminals too.  ``large``: as ``BatchSolver`` -- query graphs a plain batch
        refuses (unpruned queries on a scene of a thousand regions) run as wavefront members; small ones take the path they always took.
        ``start_boxes``, ``goal_boxes``: as ``graphs``; with a box terminal the batch is made with ``region_terminals`` (otherwise not).
        Returns one record per query: that of ``DeviceSolver.solve`` plus ``rounded_cost``, ``x_v_rounded``, ``y_v_rounded`` and
        ``graph``; with ``return_state`` also ``trace`` and ``state``, host copies of the member's trace and of its six state arrays (the
        batch and its members are closed on return).

        Replanning (gcs_admm_amd/transfer.py).  ``keep=True``: every record gains ``"snapshot"``, a ``StateSnapshot`` of the member's final
        state keyed by ``vertex_ids``, exported -- one launch for the batch -- before the members are closed; it is the caller's to
        ``close()``.  ``seed``: one snapshot or None per query; a seeded query starts its loop from the snapshot's state, matched by
        region serial (what the snapshot lacks starts at zero), at the rho its parameters say, and stops in a fraction of the
        iterations when the query moved a little.  Both work with every ``assemble``, ``prune``, ``large``, ``walk`` and terminal
        combination and across ``add_regions`` / ``remove_regions``.  Without them the call is what it always was.

        ``outside``, ``snap_radius``: as ``graphs``.  Every record has ``"snapped"``: ``{"start": None, "goal": None}``, or for a
        terminal that ``outside="snap"`` replaced ``dict(original=the point given, point=its projection, region=the key of its nearest
        region, distance=how far it moved)``.  The segment from the original point to its projection lies outside the cover: it is
        reported here and is no part of the path or of the cost."""
        from .batch import BatchSolver
        from .graph import sets_of_graph
        from .rounding import rounding_many, rounding_members, rounding_problem
        if walk not in ("host", "device"):
            raise ValueError(f"walk must be 'host' or 'device', not {walk!r}")
        graphs, info = self._graphs(starts, goals, 1e-6, 1e-9, assemble, prune, restrict, start_boxes, goal_boxes, outside, snap_radius)
        seeds = [0] * len(graphs) if seeds is None else list(seeds)
        if len(seeds) != len(graphs):
            raise ValueError("one seed per query")
        if seed is not None and len(seed) != len(graphs):
            raise ValueError("one snapshot or None per query")
        ids = [self.vertex_ids(g) for g in graphs] if keep or seed is not None else None
        # the bound's path with its restriction: one more candidate of the rounding step
        extra = info and [[(r["bound"], list(r["restriction"]), r["restriction"])] if r["restriction"] is not None else [] for r in info]
        batch = BatchSolver(graphs, state_dtype, device=self.device, large=large, region_terminals=start_boxes is not None or goal_boxes is not None)

        def close():
            batch.close()
            for m in batch.members:
                m.close()

        def attach(records):
            snapshots = batch.export_state(ids) if keep else [None] * len(graphs)
            for rec, m, g, snap in zip(records, batch.members, graphs, snapshots):
                if keep:
                    rec["snapshot"] = snap
                rec["graph"] = g
                if return_state:
                    rec["trace"] = m.trace.cpu().numpy()
                    rec["state"] = {k: getattr(m, k).cpu().numpy() for k in ("copy", "mu", "zedge", "xv", "zv", "yv")}
        with contextlib.ExitStack() as members_open:
            members_open.callback(close)
            records = batch.solve(params=params, **common) if seed is None else batch.solve(params=params, seed=list(seed), vertex_ids=ids, **common)
            if walk == "device":         # the walks read the activations where the members hold them
                rounded = rounding_members(batch.members, graphs, N=N, M=M, seeds=seeds, device=self.device, extra=extra)
                attach(records)
            else:                        # the host walks read a copy of them; the batch is closed before the rounding
                problems = [rounding_problem(m, *sets_of_graph(g), seed=s) for m, g, s in zip(batch.members, graphs, seeds)]
                attach(records)
                members_open.close()
                rounded = rounding_many(problems, N=N, M=M, device=self.device, extra=extra)
        for i, (rec, (cost, x_v, y_v)) in enumerate(zip(records, rounded)):
            if info is not None:
                rec.update(informed_bound=info[i]["bound"], kept_regions=int(info[i]["keep"].sum()))
            rec.update(rounded_cost=cost, x_v_rounded=x_v, y_v_rounded=y_v, snapped=self.snapped[i])
        return records
