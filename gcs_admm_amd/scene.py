"""Graph construction at scale on the device.

The reference's ``build_graph`` (utils.py:31-82) decides every ordered pair of regions with one LP feasibility solve through
Drake/MOSEK (``check_overlap``, :49-65) -- |V|^2 host solves, which caps it at a few hundred regions.  Here:

  1. Chebyshev centres and axis-aligned bounding boxes of all regions: batched tiny LPs on the MI355X (csrc/polytope_lp.hip);
  2. broad phase: sort-and-sweep over the first coordinate of the boxes, which leaves only pairs whose boxes touch;
  3. narrow phase on the device: one LP per candidate pair, the same decision as the reference's feasibility solve (closed sets,
     touching counts);
  4. edges in the reference's double-loop order, both directions of every intersecting pair.

``build_graph_arrays_device`` is the one pipeline: it acts on the LP statuses and makes the edge arrays.  Its two broad phases differ
only in the calls that produce centres, box statuses and the decided pair list:

  * ``"host"``: a ``PolytopeScene`` -- the batch calls ``gcsadmm_polytope_*``, arrays up and down around every step, and the sweep in
    numpy (``candidate_pairs``);
  * ``"device"``: a ``DeviceScene`` -- the regions uploaded once (``gcsadmm_scene_*``); centres, boxes and pairs never come back to
    the host between the steps, and the sweep is a kernel (``sweep_kernel``) that returns the pair list of ``candidate_pairs``
    element for element.

Both run the same three LP stages of polytope_lp.hip.  ``build_graph_device`` and ``graph_from_sets_device`` are front ends that turn
region keys into indices and back.

It raises if the HIP library or a device is missing.  The only host LPs this module ever runs are re-decisions of overlap LPs that
hit their iteration limit.  The host functions of ``gcs_admm_amd.graph`` (scipy LPs) remain what the small reference cases are built
with.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Hashable, Sequence, Tuple

import numpy as np

from . import abi
from .abi import GcsAdmmError
from .graph import GcsGraph, _finish_graph

__all__ = ["PolytopeScene", "DeviceScene", "build_graph_device", "build_graph_arrays_device", "edge_arrays", "graph_from_sets_device"]


def _call(lib, name, *args):
    """the one call into the library (prototypes: abi.PROTOTYPES; arrays go in as addresses); a status other than 0 raises GcsAdmmError"""
    rc = getattr(lib, name)(*args)
    abi.check(rc, lambda: f"{name}: {lib.gcsadmm_polytope_last_error().decode()} (status {rc})")


class PolytopeScene:
    """Regions ``A_p x <= b_p`` (p = 0..P-1) as one CSR, with the device LP entry points."""

    def __init__(self, polys: Sequence[Tuple[np.ndarray, np.ndarray]], device: int = 0):
        self.n = int(np.asarray(polys[0][0]).shape[1])
        self.P = len(polys)
        self.ptr = np.zeros(self.P + 1, np.int32)
        self.ptr[1:] = np.cumsum([np.asarray(A).shape[0] for A, _ in polys])
        self.A = np.ascontiguousarray(np.vstack([np.asarray(A, float).reshape(-1, self.n) for A, _ in polys]))
        self.b = np.ascontiguousarray(np.hstack([np.asarray(b, float).ravel() for _, b in polys]))
        self.device = int(device)
        self.lib = abi.load_library()
        self._centers = None

    def _csr(self):
        return self.n, self.P, self.ptr.ctypes.data, self.A.ctypes.data, self.b.ctypes.data

    def centers(self):
        """(centres [P, n], radii [P], LP status [P])."""
        cen = np.empty((self.P, self.n)); rad = np.empty(self.P); st = np.empty(self.P, np.int32)
        _call(self.lib, "gcsadmm_polytope_centers", *self._csr(), self.device, cen.ctypes.data, rad.ctypes.data, st.ctypes.data)
        self._centers = cen
        return cen, rad, st

    def bounds(self, centers=None):
        """(lo [P, n], hi [P, n], LP status [P, 2n]), as the LPs left them.  ``centers`` must be strictly inside their regions (the
        LPs start there): a side started from a point that is outside, or not finite, reports status -1."""
        cen = np.ascontiguousarray(centers if centers is not None else (self._centers if self._centers is not None else self.centers()[0]))
        lo = np.empty((self.P, self.n)); hi = np.empty((self.P, self.n)); st = np.empty((self.P, 2 * self.n), np.int32)
        _call(self.lib, "gcsadmm_polytope_bounds", *self._csr(), cen.ctypes.data, self.device, lo.ctypes.data, hi.ctypes.data, st.ctypes.data)
        return lo, hi, st

    def overlaps(self, pair_a, pair_b, tol: float = 1e-9, centers=None):
        """uint8 flags [num_pairs] and LP status: do regions pair_a[t], pair_b[t] intersect?

        ``centers`` [P, n] are start points only (the LP of pair t starts at ``centers[pair_a[t]]``) and need not be centres; a
        row with a NaN or an inf in it is not used: that LP starts from the least-squares point of its rows, as all do with
        ``centers=None``.  Status 0: converged, decided on ``r* >= -tol``; 1 / 2: decided early (a point with a ball around it /
        a dual bound below ``-tol``); -1: iteration limit or a non-finite iterate -- the flag of such a pair is not a decision
        (``build_graph_device`` decides it again on the host).  A non-finite result is never reported with a status >= 0."""
        pa = np.ascontiguousarray(pair_a, np.int32); pb = np.ascontiguousarray(pair_b, np.int32)
        out = np.zeros(len(pa), np.uint8); st = np.zeros(len(pa), np.int32)
        cen = centers if centers is not None else self._centers
        cen = np.ascontiguousarray(cen) if cen is not None else None
        _call(self.lib, "gcsadmm_polytope_overlaps", *self._csr(), cen.ctypes.data if cen is not None else None, len(pa), pa.ctypes.data,
              pb.ctypes.data, tol, self.device, out.ctypes.data, st.ctypes.data)
        return out, st


# A bounds LP returns an interior iterate, so a box is always slightly too small: the sweep pads every box by this much.  The boxes
# must therefore be short by (much) less than the pad -- tests/lp_cases.py holds them to a tenth of it.
SWEEP_PAD = 1e-7


def candidate_pairs(lo: np.ndarray, hi: np.ndarray, pad: float = SWEEP_PAD):
    """Unordered pairs (i < j) whose padded boxes intersect: sort on the first coordinate, sweep with a
    vectorised window per box (numpy searchsorted), test the remaining coordinates on the candidates."""
    P = lo.shape[0]
    order = np.argsort(lo[:, 0], kind="stable")
    los = lo[order, 0]
    # box order[k] can meet later boxes order[k+1 .. end_k) only: those whose lo_0 <= hi_0 + pad
    end = np.searchsorted(los, hi[order, 0] + pad, side="right")
    cnt = np.maximum(end - np.arange(P) - 1, 0)
    tot = int(cnt.sum())
    if tot == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    first = np.repeat(np.arange(P), cnt)
    offs = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    second = first + 1 + offs
    i = order[first]; j = order[second]
    keep = np.all(lo[i, 1:] <= hi[j, 1:] + pad, axis=1) & np.all(lo[j, 1:] <= hi[i, 1:] + pad, axis=1)
    i, j = i[keep], j[keep]
    a = np.minimum(i, j).astype(np.int32); b = np.maximum(i, j).astype(np.int32)
    return a, b


class DeviceScene:
    """The regions of a ``PolytopeScene`` resident on the device (``gcsadmm_scene``): uploaded once; the centres, the boxes and the
    pair list stay there between the calls, and the broad phase runs there.  Call order: ``centers``, ``bounds`` (or ``set_boxes``),
    ``candidate_pairs``, ``overlaps``, ``pairs``; a decided scene then takes ``add_regions`` and ``remove_regions`` in any order.  There is
    no CPU fallback.  Release with ``close()`` or use as a context manager."""

    def __init__(self, polys: Sequence[Tuple[np.ndarray, np.ndarray]], device: int = 0):
        host = PolytopeScene(polys, device)
        self.n, self.P, self.device, self.lib = host.n, host.P, host.device, host.lib
        self.num_pairs = 0
        self._decided = False
        self._h = C.c_void_p()
        _call(self.lib, "gcsadmm_scene_create", *host._csr(), self.device, C.byref(self._h))

    def _call(self, name, *args):
        if not self._h:
            raise GcsAdmmError("the scene is closed")
        _call(self.lib, name, self._h, *args)

    def close(self):
        if self._h:
            self._call("gcsadmm_scene_destroy")
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def centers(self):
        """(centres [P, n], radii [P], LP status [P]); the centres stay on the device for ``bounds`` and ``overlaps``."""
        cen = np.empty((self.P, self.n)); rad = np.empty(self.P); st = np.empty(self.P, np.int32)
        self._call("gcsadmm_scene_centers", cen.ctypes.data, rad.ctypes.data, st.ctypes.data)
        return cen, rad, st

    def bounds(self):
        """(lo [P, n], hi [P, n], LP status [P, 2n]) from the resident centres.  A side whose LP reports status < 0 comes back, and
        stays on the device, opened to -inf / +inf (the rule of ``build_graph_arrays_device``)."""
        lo = np.empty((self.P, self.n)); hi = np.empty((self.P, self.n)); st = np.empty((self.P, 2 * self.n), np.int32)
        self._call("gcsadmm_scene_bounds", lo.ctypes.data, hi.ctypes.data, st.ctypes.data)
        self._decided = False
        return lo, hi, st

    def set_boxes(self, lo, hi):
        """Replace the resident boxes; a NaN or ``lo > hi`` is refused."""
        lo = np.ascontiguousarray(lo, float); hi = np.ascontiguousarray(hi, float)
        if lo.shape != (self.P, self.n) or hi.shape != (self.P, self.n):
            raise ValueError(f"boxes must be [{self.P}, {self.n}]")
        self._call("gcsadmm_scene_set_boxes", lo.ctypes.data, hi.ctypes.data)
        self._decided = False

    def candidate_pairs(self, pad: float = SWEEP_PAD) -> int:
        """Broad phase on the device; returns the number of pairs.  The list (``pairs``) is that of ``candidate_pairs(lo, hi, pad)``
        on the resident boxes, element for element.  Returns after the device has finished."""
        num = C.c_int64(0)
        self._decided = False
        self._call("gcsadmm_scene_candidate_pairs", float(pad), C.addressof(num))
        self.num_pairs = int(num.value)
        return self.num_pairs

    def overlaps(self, tol: float = 1e-9):
        """Narrow phase on the resident pairs, each LP started at the resident centre of its first region: (pairs that overlap, pairs
        whose LP reports status < 0 -- their flag is not a decision)."""
        over = C.c_int64(0); und = C.c_int64(0)
        self._call("gcsadmm_scene_overlaps", float(tol), C.addressof(over), C.addressof(und))
        self._decided = True
        return int(over.value), int(und.value)

    def pairs(self):
        """(pair_a, pair_b, flags, status) of the resident pair list, a < b; flags and status are None before ``overlaps``."""
        T = self.num_pairs
        pa = np.empty(T, np.int32); pb = np.empty(T, np.int32)
        flags = np.empty(T, np.uint8) if self._decided else None
        st = np.empty(T, np.int32) if self._decided else None
        self._call("gcsadmm_scene_read_pairs", pa.ctypes.data, pb.ctypes.data, flags.ctypes.data if self._decided else None,
                   st.ctypes.data if self._decided else None)
        return pa, pb, flags, st


    def restrict_paths(self, paths, start, tol: float = 1e-10, max_iter: int = 100):
        """The convex restriction along every path of ``paths`` (sequences of region indices, in order), all in one launch
        (``gcsadmm_scene_restrict_paths``): path p has ``len(paths[p]) + 1`` points, point j in regions j - 1 and j of the path.
        ``start[p]`` [k_p + 1, n] are start points strictly inside their rows.  Returns (points: a list of [k_p + 1, n] arrays, cost
        [num_paths], Newton iterations, status): status 0 converged, 1 a start point is not strictly inside (an infeasible path), -1
        failed; the cost is the polyline length, ``inf`` unless the status is 0.  Needs none of the other calls to have run."""
        num = len(paths)
        ptr = np.zeros(num + 1, np.int32)
        ptr[1:] = np.cumsum([len(p) for p in paths])
        poly = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int64).ravel() for p in paths]) if num else np.zeros(0), np.int32)
        x0 = np.ascontiguousarray(np.concatenate([np.asarray(s, float).reshape(-1, self.n) for s in start]) if num else np.zeros((0, self.n)))
        if x0.shape[0] != int(ptr[-1]) + num:
            raise ValueError("start needs len(path) + 1 points for every path")
        pts = np.empty_like(x0); cost = np.empty(num); its = np.empty(num, np.int32); st = np.empty(num, np.int32)
        self._call("gcsadmm_scene_restrict_paths", num, ptr.ctypes.data, poly.ctypes.data, x0.ctypes.data, float(tol), int(max_iter),
                   pts.ctypes.data, cost.ctypes.data, its.ctypes.data, st.ctypes.data)
        return [pts[int(ptr[p]) + p:int(ptr[p + 1]) + p + 1] for p in range(num)], cost, its, st

    def locate(self, points, eps: float = 1e-6, tol: float = 1e-9):
        """The regions under each of ``points`` [Q, n] (``gcsadmm_scene_locate_points``, csrc/point_locate_core.h has the rule): a point
        p stands for the box ``[p - eps, p + eps]``.  Returns ``(hit_ptr int64 [Q + 1], hit_region int32, hit_class uint8)``: the hits of
        point q are ``hit_region[hit_ptr[q]:hit_ptr[q + 1]]``, region indices ascending, each of class 1 (IN: p lies in the region) or 2
        (UNDECIDED: within about eps of a facet or just beyond a vertex; a pair LP decides it).  A region that is not listed does not
        meet the box.  Needs none of the other calls to have run and leaves their resident results as they are."""
        pts = np.ascontiguousarray(points, float).reshape(-1, self.n)
        Q = pts.shape[0]
        num = C.c_int64(0)
        self._call("gcsadmm_scene_locate_points", Q, pts.ctypes.data, float(eps), float(tol), C.addressof(num))
        hit_ptr = np.empty(Q + 1, np.int64); hit_region = np.empty(int(num.value), np.int32); hit_class = np.empty(int(num.value), np.uint8)
        self._call("gcsadmm_scene_read_hits", hit_ptr.ctypes.data, hit_region.ctypes.data, hit_class.ctypes.data)
        return hit_ptr, hit_region, hit_class

    def locate_boxes(self, lo, hi, tol: float = 1e-9):
        """The regions that each of the boxes ``[lo[q], hi[q]]`` ([Q, n] each) meets (``gcsadmm_scene_locate_boxes``,
        csrc/box_locate_core.h has the rule).  Returns what ``locate`` returns: ``(hit_ptr int64 [Q + 1], hit_region int32, hit_class
        uint8)``, class 1 (IN: the box's centre lies in the region) or 2 (UNDECIDED: a pair LP decides it); a region that is not listed
        does not meet the box.  ``lo > hi`` in a coordinate or a non-finite bound is refused."""
        lo = np.ascontiguousarray(lo, float).reshape(-1, self.n); hi = np.ascontiguousarray(hi, float).reshape(-1, self.n)
        if lo.shape != hi.shape:
            raise ValueError("lo and hi must have one shape")
        Q = lo.shape[0]
        num = C.c_int64(0)
        self._call("gcsadmm_scene_locate_boxes", Q, lo.ctypes.data, hi.ctypes.data, float(tol), C.addressof(num))
        hit_ptr = np.empty(Q + 1, np.int64); hit_region = np.empty(int(num.value), np.int32); hit_class = np.empty(int(num.value), np.uint8)
        self._call("gcsadmm_scene_read_hits", hit_ptr.ctypes.data, hit_region.ctypes.data, hit_class.ctypes.data)
        return hit_ptr, hit_region, hit_class

    def project(self, points, radius=None, max_iter: int = 100):
        """The regions within ``radius[q]`` of each of ``points`` [Q, n] (default: every region) with the Euclidean projection of the
        point onto each (``gcsadmm_scene_project_points``, csrc/point_project_core.h has the rule): for a point that may lie in no
        region.  Returns ``(hit_ptr int64 [Q + 1], hit_region int32, hit_class uint8, distance [T], nearest [T, n], status int32 [T],
        iterations int32 [T])``: the entries of point q are ``hit_ptr[q]:hit_ptr[q + 1]``, region indices ascending, class 1 (INSIDE:
        the nearest point is the point itself, distance 0) or 2; status 0: solved and within the radius, 1: solved and beyond it, -1:
        failed (``distance`` and ``nearest`` are then no projection).  The list takes the place of the one ``locate`` or
        ``locate_boxes`` left.  Needs none of the other calls to have run and leaves their resident results as they are."""
        pts = np.ascontiguousarray(points, float).reshape(-1, self.n)
        Q = pts.shape[0]
        rad = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, float), (Q,)))
        num = C.c_int64(0)
        self._call("gcsadmm_scene_project_points", Q, pts.ctypes.data, rad.ctypes.data if rad is not None else None, int(max_iter), C.addressof(num))
        T = int(num.value)
        hit_ptr = np.empty(Q + 1, np.int64); hit_region = np.empty(T, np.int32); hit_class = np.empty(T, np.uint8)
        distance = np.empty(T); nearest = np.empty((T, self.n)); status = np.empty(T, np.int32); iterations = np.empty(T, np.int32)
        self._call("gcsadmm_scene_read_hits", hit_ptr.ctypes.data, hit_region.ctypes.data, hit_class.ctypes.data)
        self._call("gcsadmm_scene_read_projections", distance.ctypes.data, nearest.ctypes.data, status.ctypes.data, iterations.ctypes.data)
        return hit_ptr, hit_region, hit_class, distance, nearest, status, iterations

    def clip_segments(self, start, end, tol: float = 1e-9):
        """The regions each segment ``start[q] + t (end[q] - start[q])``, t in [0, 1], runs through, and whether they cover it
        (``gcsadmm_scene_clip_segments``, csrc/segment_clip_core.h has the rule).  Returns ``(hit_ptr int64 [Q + 1], hit_region int32,
        hit_class uint8, t_in [T], t_out [T], status int32 [Q], reach [Q], chain_ptr int64 [Q + 1], chain_hit int32)``: the hits of
        segment q are ``hit_ptr[q]:hit_ptr[q + 1]``, region indices ascending, each with the span ``[t_in, t_out]`` of the parameters at
        which the segment lies in the region inflated by ``tol``, class 1 (WHOLE: the span is [0, 1]) or 2 (PART); status 0 (COVERED,
        ``reach == 1.0``) or 1 (GAP: no hit holds ``t = reach``); ``chain_hit[chain_ptr[q]:chain_ptr[q + 1]]`` are the positions in the
        hit list of the shortest sequence of hits that covers the segment up to ``reach``.  The list takes the place of the one
        ``locate``, ``locate_boxes`` or ``project`` left.  Needs none of the other calls to have run and leaves their resident results
        as they are."""
        p = np.ascontiguousarray(start, float).reshape(-1, self.n)
        q = np.ascontiguousarray(end, float).reshape(-1, self.n)
        if p.shape != q.shape:
            raise ValueError("one end for every start")
        Q = p.shape[0]
        num, links = C.c_int64(0), C.c_int64(0)
        self._call("gcsadmm_scene_clip_segments", Q, p.ctypes.data, q.ctypes.data, float(tol), C.addressof(num), C.addressof(links))
        T = int(num.value)
        hit_ptr = np.empty(Q + 1, np.int64); hit_region = np.empty(T, np.int32); hit_class = np.empty(T, np.uint8)
        t_in = np.empty(T); t_out = np.empty(T); status = np.empty(Q, np.int32); reach = np.empty(Q)
        chain_ptr = np.empty(Q + 1, np.int64); chain_hit = np.empty(int(links.value), np.int32)
        self._call("gcsadmm_scene_read_hits", hit_ptr.ctypes.data, hit_region.ctypes.data, hit_class.ctypes.data)
        self._call("gcsadmm_scene_read_spans", t_in.ctypes.data, t_out.ctypes.data)
        self._call("gcsadmm_scene_read_cover", status.ctypes.data, reach.ctypes.data, chain_ptr.ctypes.data, chain_hit.ctypes.data)
        return hit_ptr, hit_region, hit_class, t_in, t_out, status, reach, chain_ptr, chain_hit

    def regions(self):
        """The resident results per region as they are, no LP run (``gcsadmm_scene_read_regions``; after ``centers`` and ``bounds``):
        ``(centres [P, n], radii [P], LP status [P], lo [P, n], hi [P, n], LP status [P, 2n])``."""
        cen = np.empty((self.P, self.n)); rad = np.empty(self.P); st_c = np.empty(self.P, np.int32)
        lo = np.empty((self.P, self.n)); hi = np.empty((self.P, self.n)); st_b = np.empty((self.P, 2 * self.n), np.int32)
        self._call("gcsadmm_scene_read_regions", cen.ctypes.data, rad.ctypes.data, st_c.ctypes.data, lo.ctypes.data, hi.ctypes.data, st_b.ctypes.data)
        return cen, rad, st_c, lo, hi, st_b

    def add_regions(self, polys, pad: float = SWEEP_PAD, tol: float = 1e-9):
        """Append ``polys`` to a decided scene (``gcsadmm_scene_add_regions``; after ``overlaps``) as regions ``P .. P + len(polys) - 1``.
        Only the LPs of the new regions and of the pairs they form run; afterwards every resident result is that of a scene created
        on the whole list (``pad``, ``tol``: those of ``candidate_pairs`` and ``overlaps``).  Returns ``(centres [K, n], radii [K], LP
        status [K], counts)`` of the new regions, ``counts = dict(new_pairs, overlapping, undecided)`` of the new pairs.  A new region
        whose centre LP reports status < 0 or whose radius is <= 0 is refused, the scene unchanged: the GcsAdmmError carries
        ``results = (centres, radii, status)``."""
        K = len(polys)
        ptr = np.zeros(K + 1, np.int32)
        ptr[1:] = np.cumsum([np.asarray(A).shape[0] for A, _ in polys])
        A = np.ascontiguousarray(np.vstack([np.asarray(A, float).reshape(-1, self.n) for A, _ in polys])) if K else np.zeros((0, self.n))
        b = np.ascontiguousarray(np.hstack([np.asarray(b, float).ravel() for _, b in polys])) if K else np.zeros(0)
        cen = np.zeros((K, self.n)); rad = np.ones(K); st = np.zeros(K, np.int32)
        new = C.c_int64(0); over = C.c_int64(0); und = C.c_int64(0)
        try:
            self._call("gcsadmm_scene_add_regions", K, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, float(pad), float(tol), cen.ctypes.data,
                       rad.ctypes.data, st.ctypes.data, C.addressof(new), C.addressof(over), C.addressof(und))
        except GcsAdmmError as e:
            e.results = (cen, rad, st)
            raise
        self.P += K
        self.num_pairs += int(new.value)
        return cen, rad, st, dict(new_pairs=int(new.value), overlapping=int(over.value), undecided=int(und.value))

    def remove_regions(self, indices):
        """Take the regions ``indices`` (distinct, in range) out of the scene, in any state of it (``gcsadmm_scene_remove_regions``):
        the others keep their order and are renumbered without gaps, and what is resident is compacted -- a pair stays iff both its
        regions stay.  Returns the length of the pair list afterwards."""
        idx = np.ascontiguousarray(indices, np.int32).ravel()
        left = C.c_int64(0)
        self._call("gcsadmm_scene_remove_regions", len(idx), idx.ctypes.data, C.addressof(left))
        self.P -= len(idx)
        self.num_pairs = int(left.value)
        return self.num_pairs

    def build_region_graph(self, flags=None) -> int:
        """The region graph of the decided pairs, made and kept on the device (``gcsadmm_scene_build_region_graph``; after ``overlaps``):
        ``edge_arrays(pa, pb, flags)`` with its rows and reverse edges, without a sort.  ``flags``: host decisions [num_pairs] that take
        the place of the resident flags for this graph (default: the resident flags).  Returns the number of directed edges.  A new
        ``candidate_pairs`` or ``overlaps`` and every edit end the graph."""
        f = None if flags is None else np.ascontiguousarray(flags, np.uint8).ravel()
        if f is not None and len(f) != self.num_pairs:
            raise ValueError(f"flags must be [{self.num_pairs}]")
        num = C.c_int64(0)
        self._call("gcsadmm_scene_build_region_graph", f.ctypes.data if f is not None else None, C.addressof(num))
        self.num_region_edges = int(num.value)
        return self.num_region_edges

    def region_graph(self):
        """``(row_ptr int64 [P + 1], edge_tail, edge_head, reverse int32 [E_R])`` of the resident region graph: the edges with tail u are
        ``row_ptr[u]:row_ptr[u + 1]``, heads ascending; ``reverse[p]`` is the id of the opposite edge."""
        row_ptr = np.empty(self.P + 1, np.int64)
        self._call("gcsadmm_scene_read_region_graph", row_ptr.ctypes.data, None, None, None)
        E = int(row_ptr[-1])
        tail = np.empty(E, np.int32); head = np.empty(E, np.int32); rev = np.empty(E, np.int32)
        self._call("gcsadmm_scene_read_region_graph", None, tail.ctypes.data, head.ctypes.data, rev.ctypes.data)
        return row_ptr, tail, head, rev

    def query_graphs(self, term_ptr, term_region, st_adjacent, chunk_queries: int = 0):
        """The index arrays of the query graphs of a batch from one kernel (``gcsadmm_scene_query_graphs``; csrc/query_graph_core.h has
        the rule; after ``build_region_graph``).  ``B = len(st_adjacent)`` queries; points ``0 .. B-1`` are the starts and ``B .. 2B-1``
        the goals, point q lies in the regions ``term_region[term_ptr[q]:term_ptr[q + 1]]`` (ascending), ``st_adjacent[i]`` says whether
        the two point boxes of query i meet.  Returns one tuple ``(edge_tail, edge_head, inc_ptr, inc_edge, inc_out, edge_inc_tail,
        edge_inc_head)`` per query, int32 views into seven flat arrays: what ``graph._finish_graph`` makes of the merged edge list, vertex
        0 the start, 1 the goal, r + 2 region r.  ``chunk_queries``: queries per launch (0: the library bounds its workspace)."""
        return query_graph_views(self.P, self.num_region_edges, term_ptr, term_region, st_adjacent,
                                 lambda *arrays: self._call("gcsadmm_scene_query_graphs", *arrays), chunk_queries)


    def region_paths(self, points, term_ptr, term_region, max_len=None):
        """One candidate path per query: a shortest path on the resident region graph under the distances between centres
        (``gcsadmm_scene_region_paths``; csrc/informed_core.h has the rule; after ``build_region_graph``).  ``points`` [2 B, n]: the
        starts, then the goals; ``term_ptr``, ``term_region``: as ``query_graphs``.  ``max_len``: the most regions of a path (default P).
        Returns ``(paths, cost, status)``: int32 arrays of region indices from the start side to the goal side, the length of the
        polyline through their centres, and 0 found / 1 none (empty path, cost inf) / 2 longer than ``max_len`` (empty path, its cost) /
        -1 not read back."""
        return region_path_views(self.n, self.P, points, term_ptr, term_region, max_len, lambda *arrays: self._call("gcsadmm_scene_region_paths", *arrays))

    def informed_regions(self, points, bound, pad: float = SWEEP_PAD):
        """bool [B, P]: ``keep[i, r]`` iff ``dist(s_i, box_r) + dist(g_i, box_r) <= bound[i] (1 + 1e-9)`` on the resident boxes, every
        side moved out by ``pad`` (``gcsadmm_scene_informed_regions``).  ``points`` [2 B, n]: the starts, then the goals; ``bound`` [B]:
        the length of a feasible path of each query, or ``inf`` (keeps every region)."""
        return informed_keep_array(self.n, self.P, points, bound, pad, lambda *arrays: self._call("gcsadmm_scene_informed_regions", *arrays))

    def region_paths_sets(self, lo, hi, term_ptr, term_region, max_len=None):
        """``region_paths`` between start and goal SETS (``gcsadmm_scene_region_paths_sets``; csrc/informed_set_core.h has the rule).
        ``lo``, ``hi`` [2 B, n]: the start boxes, then the goal boxes (a point: ``lo == hi``, and the results have the bits of
        ``region_paths``); ``term_ptr``, ``term_region``: the regions that meet each box.  The distance of a centre to the box takes the
        place of the distance to the point, and the search ends once nothing below the cheapest goal cost moves.  Returns what
        ``region_paths`` returns."""
        return region_path_set_views(self.n, self.P, lo, hi, term_ptr, term_region, max_len,
                                     lambda *arrays: self._call("gcsadmm_scene_region_paths_sets", *arrays))

    def informed_regions_sets(self, lo, hi, bound, pad: float = SWEEP_PAD):
        """bool [B, P]: ``keep[i, r]`` iff ``gap(S_i, box_r) + gap(G_i, box_r) <= bound[i] (1 + 1e-9)``, the distances between the
        terminal boxes and the resident boxes, every side of those moved out by ``pad`` (``gcsadmm_scene_informed_regions_sets``).
        ``lo``, ``hi`` [2 B, n]: as ``region_paths_sets``; ``bound`` [B]: the length of a feasible path of each query, finite."""
        return informed_keep_set_array(self.n, self.P, lo, hi, bound, pad, lambda *arrays: self._call("gcsadmm_scene_informed_regions_sets", *arrays))

    def induced_sizes(self, keep, term_ptr, term_region, st_adjacent):
        """``(num_kept int32 [B], num_edges int64 [B])`` of the graphs ``induced_query_graphs`` would write (``gcsadmm_scene_induced_sizes``:
        the counts alone)"""
        return induced_size_arrays(self.P, keep, term_ptr, term_region, st_adjacent, lambda *arrays: self._call("gcsadmm_scene_induced_sizes", *arrays))[4:]

    def induced_query_graphs(self, keep, term_ptr, term_region, st_adjacent, chunk_queries: int = 0):
        """The index arrays of the query graphs of a batch, each on its own kept regions (``gcsadmm_scene_induced_sizes``, then
        ``gcsadmm_scene_induced_query_graphs``; csrc/induced_graph_core.h has the rule; after ``build_region_graph``).  ``keep`` [B, P]:
        non-zero keeps region r for query i (every hit region must be kept); the other arguments as ``query_graphs``, in scene indices.
        Returns one tuple of seven int32 views per query, as ``query_graphs``: vertex 0 the start, 1 the goal, j + 2 the j-th kept region
        in scene order; ``inc_ptr`` has ``kept + 3`` entries."""
        return induced_query_graph_views(self.P, keep, term_ptr, term_region, st_adjacent,
                                         lambda *arrays: self._call("gcsadmm_scene_induced_sizes", *arrays),
                                         lambda *arrays: self._call("gcsadmm_scene_induced_query_graphs", *arrays), chunk_queries)


def region_path_views(n, P, points, term_ptr, term_region, max_len, call):
    """the arrays of ``gcsadmm_scene_region_paths`` around ``call(num_queries, points, term_ptr, term_region, max_len, *four outputs)``
    (addresses), the paths cut to their lengths"""
    pts = np.ascontiguousarray(points, float).reshape(-1, n)
    ptr = np.ascontiguousarray(term_ptr, np.int64).ravel()
    reg = np.ascontiguousarray(term_region, np.int32).ravel()
    B = pts.shape[0] // 2
    if pts.shape[0] != 2 * B or len(ptr) != 2 * B + 1:
        raise ValueError("points needs 2 B rows and term_ptr 2 B + 1 entries: the starts, then the goals")
    max_len = max(int(P), 1) if max_len is None else int(max_len)
    path = np.full((B, max(max_len, 0)), -1, np.int32); length = np.zeros(B, np.int32); cost = np.full(B, np.inf); status = np.full(B, 1, np.int32)
    call(B, pts.ctypes.data, ptr.ctypes.data, reg.ctypes.data, max_len, path.ctypes.data, length.ctypes.data, cost.ctypes.data, status.ctypes.data)
    return [path[i, :length[i]] if status[i] == 0 else path[i, :0] for i in range(B)], cost, status


def informed_keep_array(n, P, points, bound, pad, call):
    """the arrays of ``gcsadmm_scene_informed_regions`` around ``call(num_queries, points, bound, pad, keep, num_kept)`` (addresses)"""
    pts = np.ascontiguousarray(points, float).reshape(-1, n)
    bnd = np.ascontiguousarray(bound, float).ravel()
    B = len(bnd)
    if pts.shape[0] != 2 * B:
        raise ValueError("points needs 2 B rows: the starts, then the goals")
    keep = np.zeros((B, P), np.uint8)
    call(B, pts.ctypes.data, bnd.ctypes.data, float(pad), keep.ctypes.data, None)
    return keep != 0


def _terminal_boxes(n, lo, hi):
    lo = np.ascontiguousarray(lo, float).reshape(-1, n); hi = np.ascontiguousarray(hi, float).reshape(-1, n)
    if lo.shape != hi.shape or lo.shape[0] % 2:
        raise ValueError("lo and hi need 2 B rows each: the start boxes, then the goal boxes")
    return lo, hi


def region_path_set_views(n, P, lo, hi, term_ptr, term_region, max_len, call):
    """the arrays of ``gcsadmm_scene_region_paths_sets`` around ``call(num_queries, lo, hi, term_ptr, term_region, max_len, *four
    outputs)`` (addresses): ``region_path_views`` with the two box arrays in the place of the points"""
    lo, hi = _terminal_boxes(n, lo, hi)
    return region_path_views(n, P, lo, term_ptr, term_region, max_len, lambda B, _, *rest: call(B, lo.ctypes.data, hi.ctypes.data, *rest))


def informed_keep_set_array(n, P, lo, hi, bound, pad, call):
    """the arrays of ``gcsadmm_scene_informed_regions_sets`` around ``call(num_queries, lo, hi, bound, pad, keep, num_kept)`` (addresses)"""
    lo, hi = _terminal_boxes(n, lo, hi)
    return informed_keep_array(n, P, lo, bound, pad, lambda B, _, *rest: call(B, lo.ctypes.data, hi.ctypes.data, *rest))


def query_graph_views(P, region_edges, term_ptr, term_region, st_adjacent, call, chunk_queries=0):
    """the flat arrays of ``gcsadmm_scene_query_graphs`` around ``call(num_queries, term_ptr, term_region, st_adjacent, chunk_queries,
    edge_off, *seven outputs)`` (addresses), cut into one tuple of views per query"""
    ptr = np.ascontiguousarray(term_ptr, np.int64).ravel()
    reg = np.ascontiguousarray(term_region, np.int32).ravel()
    st = np.ascontiguousarray(st_adjacent, np.uint8).ravel()
    B = len(st)
    if len(ptr) != 2 * B + 1:
        raise ValueError("term_ptr needs 2 B + 1 entries: the starts, then the goals")
    hits = np.diff(ptr)
    edge_off = np.zeros(B + 1, np.int64)
    edge_off[1:] = np.cumsum(region_edges + 2 * (hits[:B] + hits[B:]) + 2 * (st != 0))
    E = int(edge_off[-1])
    edge = [np.empty(E, np.int32) for _ in range(4)]            # edge_tail, edge_head, edge_inc_tail, edge_inc_head
    inc = [np.empty(2 * E, np.int32) for _ in range(2)]         # inc_edge, inc_out
    inc_ptr = np.empty(B * (P + 3), np.int32)
    flat = (edge[0], edge[1], inc_ptr, inc[0], inc[1], edge[2], edge[3])
    call(B, ptr.ctypes.data, reg.ctypes.data, st.ctypes.data, int(chunk_queries), edge_off.ctypes.data, *(a.ctypes.data for a in flat))
    out = []
    for i in range(B):
        e0, e1 = int(edge_off[i]), int(edge_off[i + 1])
        cut = (slice(e0, e1), slice(e0, e1), slice(i * (P + 3), (i + 1) * (P + 3)), slice(2 * e0, 2 * e1), slice(2 * e0, 2 * e1), slice(e0, e1),
               slice(e0, e1))
        out.append(tuple(a[c] for a, c in zip(flat, cut)))
    return out


def induced_size_arrays(P, keep, term_ptr, term_region, st_adjacent, sizes_call):
    """the arrays of ``gcsadmm_scene_induced_sizes`` around ``sizes_call(num_queries, keep, term_ptr, term_region, st_adjacent, num_kept,
    num_edges)`` (addresses): the four inputs as the call takes them, then ``num_kept`` int32 [B] and ``num_edges`` int64 [B]"""
    ptr = np.ascontiguousarray(term_ptr, np.int64).ravel()
    reg = np.ascontiguousarray(term_region, np.int32).ravel()
    st = np.ascontiguousarray(st_adjacent, np.uint8).ravel()
    B = len(st)
    if len(ptr) != 2 * B + 1:
        raise ValueError("term_ptr needs 2 B + 1 entries: the starts, then the goals")
    flags = np.ascontiguousarray(np.asarray(keep).reshape(B, P), np.uint8)      # (bool or uint8: any non-zero byte keeps)
    num_kept = np.zeros(B, np.int32); num_edges = np.zeros(B, np.int64)
    sizes_call(B, flags.ctypes.data, ptr.ctypes.data, reg.ctypes.data, st.ctypes.data, num_kept.ctypes.data, num_edges.ctypes.data)
    return flags, ptr, reg, st, num_kept, num_edges


def induced_query_graph_views(P, keep, term_ptr, term_region, st_adjacent, sizes_call, graphs_call, chunk_queries=0):
    """the flat arrays of ``gcsadmm_scene_induced_query_graphs`` around ``sizes_call(num_queries, keep, term_ptr, term_region,
    st_adjacent, num_kept, num_edges)`` and ``graphs_call(num_queries, keep, term_ptr, term_region, st_adjacent, chunk_queries,
    vertex_off, edge_off, *seven outputs)`` (addresses): the sizes first, then arrays laid out by them, cut into one tuple of views per
    query (its ``inc_ptr`` has ``num_kept + 3`` entries)"""
    flags, ptr, reg, st, num_kept, num_edges = induced_size_arrays(P, keep, term_ptr, term_region, st_adjacent, sizes_call)
    B = len(st)
    vertex_off = np.zeros(B + 1, np.int64); edge_off = np.zeros(B + 1, np.int64)
    vertex_off[1:] = np.cumsum(num_kept.astype(np.int64) + 3); edge_off[1:] = np.cumsum(num_edges)
    E, V = int(edge_off[-1]), int(vertex_off[-1])
    edge = [np.empty(E, np.int32) for _ in range(4)]            # edge_tail, edge_head, edge_inc_tail, edge_inc_head
    inc = [np.empty(2 * E, np.int32) for _ in range(2)]         # inc_edge, inc_out
    inc_ptr = np.empty(V, np.int32)
    flat = (edge[0], edge[1], inc_ptr, inc[0], inc[1], edge[2], edge[3])
    graphs_call(B, flags.ctypes.data, ptr.ctypes.data, reg.ctypes.data, st.ctypes.data, int(chunk_queries), vertex_off.ctypes.data,
                edge_off.ctypes.data, *(a.ctypes.data for a in flat))
    out = []
    for i in range(B):
        e0, e1 = int(edge_off[i]), int(edge_off[i + 1])
        cut = (slice(e0, e1), slice(e0, e1), slice(int(vertex_off[i]), int(vertex_off[i + 1])), slice(2 * e0, 2 * e1), slice(2 * e0, 2 * e1),
               slice(e0, e1), slice(e0, e1))
        out.append(tuple(a[c] for a, c in zip(flat, cut)))
    return out


def check_centres(rad, st_c, name=lambda idx: idx.tolist()):
    """the rule of graph construction for centre LPs: one that did not converge raises GcsAdmmError, a region without interior ValueError"""
    if np.any(st_c < 0):
        raise GcsAdmmError(f"centre LP did not converge for regions {name(np.nonzero(st_c < 0)[0][:8])} (of {int((st_c < 0).sum())})")
    if np.any(rad <= 0):
        raise ValueError(f"regions without interior: {name(np.nonzero(rad <= 0)[0][:5])}")


def edge_arrays(pa, pb, flags):
    """both directions of every intersecting pair in the reference's double-loop order (by tail, then head), int32"""
    keep = np.asarray(flags) != 0
    a = pa[keep]; b = pb[keep]
    tail = np.concatenate([a, b]); head = np.concatenate([b, a])
    o = np.lexsort((head, tail))
    return tail[o].astype(np.int32), head[o].astype(np.int32)


def build_graph_arrays_device(polys: Sequence[Tuple[np.ndarray, np.ndarray]], device: int = 0, tol: float = 1e-9, scene=None,
                              stats: dict | None = None, names: Sequence[Hashable] | None = None, broad_phase: str = "device",
                              pairs_out: dict | None = None):
    """``utils.build_graph`` (reference utils.py:31-82) with the LPs on the device, arrays in and out: ``polys[p] = (A_p, b_p)``;
    returns ``(edge_tail, edge_head, centres)``, int32 region indices in the reference's double-loop order.

    Every LP reports a status (0 converged, 1 / 2 decided early, -1 iteration limit) and none is ignored:
      * a centre LP that did not converge has no trustworthy interior point -> GcsAdmmError naming the regions;
      * a bounding-box LP that did not converge returns an INTERIOR iterate, i.e. a box that is too small, and the sweep
        would silently drop real neighbours: that side of the box is opened up (+-inf), which only adds candidates;
      * an overlap LP that did not converge is decided again by the host LP of ``graph.polytopes_overlap`` (one HiGHS
        solve per pair, the reference's own method) instead of from its unfinished iterate.
    ``stats`` (optional dict) receives the counts.  ``broad_phase``: ``"host"`` (the batch LP calls of a PolytopeScene around the numpy
    sweep) or ``"device"`` (a resident DeviceScene: no host sweep, no copies between the steps) -- the same edges.  ``scene``: a
    prepared scene of that kind (tests inject one; a DeviceScene is left open).  ``names``: what to call the regions in an error
    message (default: their indices).  ``pairs_out`` (optional dict) receives the decided pair list, host decisions included:
    ``pa``, ``pb``, ``flags``, ``status``."""
    if broad_phase not in ("host", "device"):
        raise ValueError(f"broad_phase must be 'host' or 'device', not {broad_phase!r}")
    name = (lambda idx: [names[i] for i in idx]) if names is not None else (lambda idx: idx.tolist())

    # the two call sequences to (cen, st_b, pa, pb, flags, st_o); everything after them is common
    if broad_phase == "host":
        if scene is None:
            scene = PolytopeScene(polys, device)
        cen, rad, st_c = scene.centers()
        check_centres(rad, st_c, name)
        lo, hi, st_b = scene.bounds(cen)
        # the batch call opens nothing; status layout of bounds_kernel (polytope_lp.hip): [P][n][2] = (min, max) per axis
        st_b = np.asarray(st_b).reshape(lo.shape + (2,))
        pa, pb = candidate_pairs(np.where(st_b[..., 0] < 0, -np.inf, lo), np.where(st_b[..., 1] < 0, np.inf, hi))
        flags, st_o = scene.overlaps(pa, pb, tol, cen)
    else:
        own = scene is None
        if own:
            scene = DeviceScene(polys, device)
        try:
            cen, rad, st_c = scene.centers()
            check_centres(rad, st_c, name)
            _, _, st_b = scene.bounds()          # failed sides are opened on the device
            scene.candidate_pairs()
            scene.overlaps(tol)
            pa, pb, flags, st_o = scene.pairs()
        finally:
            if own:
                scene.close()
    redo = np.nonzero(np.asarray(st_o) < 0)[0]
    if len(redo):
        from .graph import polytopes_overlap
        flags = np.array(flags, copy=True)
        for t in redo:
            (A1, b1), (A2, b2) = polys[pa[t]], polys[pb[t]]
            flags[t] = 1 if polytopes_overlap(np.asarray(A1, float), np.asarray(b1, float), np.asarray(A2, float), np.asarray(b2, float)) else 0
    if stats is not None:
        stats.update(bounds_opened=int((np.asarray(st_b) < 0).sum()), overlaps_redone_on_host=int(len(redo)), candidate_pairs=int(len(pa)))
    if pairs_out is not None:
        pairs_out.update(pa=np.asarray(pa), pb=np.asarray(pb), flags=np.asarray(flags), status=np.asarray(st_o))
    tail, head = edge_arrays(pa, pb, flags)
    return tail, head, cen


def build_graph_device(As: Dict[Hashable, np.ndarray], bs: Dict[Hashable, np.ndarray], device: int = 0, tol: float = 1e-9,
                       scene=None, stats: dict | None = None, broad_phase: str = "host"):
    """``build_graph_arrays_device`` by region key.  Returns ``(vertices, edges, I_v_in, I_v_out, centres)``; ``edges`` are key pairs in
    the reference's double-loop order.  ``scene``, ``stats``, ``broad_phase``: as there (``scene`` is a PolytopeScene for ``"host"``, a
    DeviceScene for ``"device"``); an error message names the regions by key."""
    vertices = list(As.keys())
    tail, head, cen = build_graph_arrays_device([(As[v], bs[v]) for v in vertices], device, tol, scene, stats, names=vertices, broad_phase=broad_phase)
    edges = [(vertices[t], vertices[h]) for t, h in zip(tail.tolist(), head.tolist())]
    I_v_in = {v: [] for v in vertices}
    I_v_out = {v: [] for v in vertices}
    for e in edges:
        I_v_out[e[0]].append(e)
        I_v_in[e[1]].append(e)
    return vertices, edges, I_v_in, I_v_out, cen


def graph_from_sets_device(As, bs, n, device: int = 0, broad_phase: str = "host") -> GcsGraph:
    """``graph_from_sets`` with edges and interior points from the device LPs: the edge arrays go straight into the CSR."""
    keys = list(As.keys())
    if 's' not in As or 't' not in As:
        raise KeyError("case must define vertices 's' and 't'")
    polys = [(np.asarray(As[k], float), np.asarray(bs[k], float)) for k in keys]
    tail, head, cen = build_graph_arrays_device(polys, device, names=keys, broad_phase=broad_phase)
    return _finish_graph(int(n), keys, tail, head, polys, cen, keys.index('s'), keys.index('t'))
