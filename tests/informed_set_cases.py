"""Terminal boxes, the host build and a plain-numpy restatement for the tests of the informed region set between start and goal SETS
(csrc/informed_set_core.h; gcsadmm_scene_region_paths_sets / _informed_regions_sets in csrc/polytope_lp.hip), shared by
test_informed_sets.py (host build, no GPU) and test_gpu_informed_sets.py.  The scenes, their queries and the margins are those of
informed_cases.py.

The restatement is ``informed_cases.restate_path`` with the two set distances in the place of the point distances: a heap Dijkstra that
runs to the end, with NO bound on the search -- what the bounded rule of the header must agree with in status, path and cost, and in
``d`` wherever that is at most the cost."""
from __future__ import annotations

import ctypes as C
import heapq
import os

import numpy as np

import hostemu_lib
import informed_cases as I
from gcs_admm_amd.native_build import build_library
from gcs_admm_amd.scene import SWEEP_PAD, informed_keep_set_array, region_path_set_views

EMU_SRC = os.path.join(hostemu_lib.HOSTEMU, "informed_set_emu.cpp")
HALF_WIDTHS = (0.05, 0.3, 0.9)
KINDS = ("point_box", "box_point", "box_box")
ORDERS = (0, 1, 2, 3)          # bit 0: the lanes backwards; bit 1: a round reads the bound of the round before


# ------------------------------------------------------------------------------------------- terminals
def meeting(lo, hi, tlo, thi, eps=0.0):
    """the ascending int32 list of the boxes that meet ``[tlo - eps, thi + eps]`` (closed sets), per terminal"""
    return [np.nonzero(np.all((lo <= h + eps) & (l - eps <= hi), axis=1))[0].astype(np.int32) for l, h in zip(tlo, thi)]


def batch(c, B, kind="point_point", half=0.0):
    """(tlo [2 B, n], thi [2 B, n], term_ptr, term_region) of the first B queries of case ``c``: a side named ``box`` is the box of
    half-width ``half`` around the query's point, a side named ``point`` the point as the box lo == hi, under the regions within
    ``I.EPS`` of it (the lists of ``Case.batch``)"""
    start, goal = kind.split("_")
    hs, hg = (half if start == "box" else 0.0), (half if goal == "box" else 0.0)
    tlo = np.ascontiguousarray(np.vstack([c.S[:B] - hs, c.G[:B] - hg])); thi = np.ascontiguousarray(np.vstack([c.S[:B] + hs, c.G[:B] + hg]))
    eps = np.repeat([0.0 if start == "box" else I.EPS, 0.0 if goal == "box" else I.EPS], B)
    regs = [meeting(c.lo, c.hi, tlo[q:q + 1], thi[q:q + 1], eps[q])[0] for q in range(2 * B)]
    return (tlo, thi) + I.term_lists(regs)


def wide_batch(c):
    """two queries on ``boxes300``: 0 from the start point of query 0 to a goal box that meets every region, 1 from a start box that
    meets every region to the goal point of query 2 -- lists longer than the 256 lanes"""
    whole_lo, whole_hi = c.lo.min(axis=0) - 1.0, c.hi.max(axis=0) + 1.0
    tlo = np.ascontiguousarray(np.vstack([c.S[0], whole_lo, whole_lo, c.G[2]])); thi = np.ascontiguousarray(np.vstack([c.S[0], whole_hi, whole_hi, c.G[2]]))
    regs = [meeting(c.lo, c.hi, tlo[q:q + 1], thi[q:q + 1], I.EPS if q in (0, 3) else 0.0)[0] for q in range(4)]
    assert len(regs[1]) == len(regs[2]) == c.P > 256
    return (tlo, thi) + I.term_lists(regs)


# ------------------------------------------------------------------------------------------- the restatement
def set_dist(c, tlo, thi):
    """dist(c, T): the distance of point c to the box [tlo, thi], the squares summed in ascending coordinate order"""
    sq = 0.0
    for k in range(len(c)):
        t = max(tlo[k] - c[k], 0.0, c[k] - thi[k])
        sq = sq + t * t
    return float(np.sqrt(sq))


def gap(tlo, thi, lo, hi, pad):
    """gap(T, box_r) for every region r: [P]"""
    t = np.maximum(np.maximum(lo - pad - thi, 0.0), tlo - hi - pad)
    sq = np.zeros(len(lo))
    for k in range(lo.shape[1]):
        sq = sq + t[:, k] * t[:, k]
    return np.sqrt(sq)


def restate_path(centers, row_ptr, head, w, slo, shi, glo, ghi, rs, rt, max_len=None):
    """(path, cost, status, d) of one query by the rule, the search run to the end: heap Dijkstra from init, the goal choice, the
    backtrack"""
    P = len(row_ptr) - 1
    max_len = P if max_len is None else max_len
    init = np.full(P, np.inf)
    for r in rs:
        init[r] = set_dist(centers[r], slo, shi)
    d = init.copy()
    heap = [(d[r], int(r)) for r in rs]
    heapq.heapify(heap)
    done = np.zeros(P, bool)
    while heap:
        du, u = heapq.heappop(heap)
        if done[u] or du > d[u]:
            continue
        done[u] = True
        for p in range(row_ptr[u], row_ptr[u + 1]):
            v = head[p]
            if du + w[p] < d[v]:
                d[v] = du + w[p]
                heapq.heappush(heap, (d[v], int(v)))
    cost, goal = np.inf, -1
    for r in rt:
        c = d[r] + set_dist(centers[r], glo, ghi)
        if c < cost:
            cost, goal = c, int(r)
    if goal < 0:
        return np.zeros(0, np.int32), np.inf, 1, d
    path, v = [goal], goal
    while d[v] != init[v]:
        step = [head[p] for p in range(row_ptr[v], row_ptr[v + 1]) if d[head[p]] + w[p] == d[v]]
        if not step or len(path) >= P:
            return np.zeros(0, np.int32), cost, -1, d
        v = int(min(step))
        path.append(v)
    if len(path) > max_len:
        return np.zeros(0, np.int32), cost, 2, d
    return np.array(path[::-1], np.int32), cost, 0, d


def polyline_cost(centers, slo, shi, glo, ghi, path):
    total = set_dist(centers[path[0]], slo, shi)
    for u, v in zip(path[:-1], path[1:]):
        total = total + I.dist(centers[u], centers[v])
    return total + set_dist(centers[path[-1]], glo, ghi)


def restate_keep(lo, hi, slo, shi, glo, ghi, bound, pad=SWEEP_PAD):
    """(keep bool [P], near bool [P]: the sum of the gaps within NEAR * bound of the threshold)"""
    lb = gap(slo, shi, lo, hi, pad) + gap(glo, ghi, lo, hi, pad)
    limit = bound * (1.0 + I.SLACK)
    return lb <= limit, np.abs(lb - limit) <= I.NEAR * bound


def check_paths(got, centers, row_ptr, tail, head, w, tlo, thi, term_ptr, term_region, exact=False):
    """``informed_cases.check_paths`` for box terminals: ``got = (paths, cost, status)`` of B queries against the rule and the
    restatement; returns the restatement's results"""
    paths, cost, status = got
    B = len(status)
    edges = set(zip(tail.tolist(), head.tolist()))
    n = centers.shape[1]
    ref = []
    for i in range(B):
        rs, rt = term_region[term_ptr[i]:term_ptr[i + 1]], term_region[term_ptr[B + i]:term_ptr[B + i + 1]]
        boxes = (tlo[i], thi[i], tlo[B + i], thi[B + i])
        want = restate_path(centers, row_ptr, head, w, *boxes, rs, rt)
        ref.append(want)
        assert status[i] == want[2], (i, status[i], want[2])
        if want[2] != 0:
            assert len(paths[i]) == 0 and cost[i] == np.inf
            continue
        p = paths[i]
        assert p.dtype == np.int32 and len(p) >= 1 and p[0] in rs and p[-1] in rt, (i, p)
        assert all((int(u), int(v)) in edges for u, v in zip(p[:-1], p[1:])), (i, p)
        tol = I.margin(len(p), n)
        assert abs(cost[i] - polyline_cost(centers, *boxes, p)) <= tol * cost[i], i
        assert abs(cost[i] - want[1]) <= tol * want[1], (i, cost[i], want[1])
        if exact:
            assert np.array_equal(p, want[0]), (i, p, want[0])
    return ref


def check_keep(got, lo, hi, tlo, thi, bound, pad=SWEEP_PAD):
    """bool [B, P] against the restatement; no region of these cases may be near the threshold"""
    B = len(bound)
    assert got.dtype == bool and got.shape == (B, len(lo))
    for i in range(B):
        want, near = restate_keep(lo, hi, tlo[i], thi[i], tlo[B + i], thi[B + i], bound[i], pad)
        assert not near.any(), (i, np.nonzero(near)[0])
        assert np.array_equal(got[i], want), (i, np.nonzero(got[i] != want)[0])


def check_distances(d, ref):
    """the distances a bounded search left against the restatement's result ``ref``: the fixed point wherever that is at most the
    cost, and never below it"""
    want, cost = ref[3], ref[1]
    settled = want <= cost
    assert d[settled].tobytes() == want[settled].tobytes()
    assert np.all(d >= want)


# ------------------------------------------------------------------------------------------- the host build
_p, _i, _d = C.c_void_p, C.c_int, C.c_double


def declare(lib):
    lib.inf_set_emu_last_error.restype = C.c_char_p
    lib.inf_set_emu_last_error.argtypes = []
    lib.inf_set_emu_dist.restype = _d
    lib.inf_set_emu_dist.argtypes = [_i, _p, _p, _p]
    lib.inf_set_emu_gap.restype = _d
    lib.inf_set_emu_gap.argtypes = [_i, _p, _p, _p, _p, _d]
    lib.inf_set_emu_paths.restype = _i
    lib.inf_set_emu_paths.argtypes = [_i, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p, _i, _i] + [_p] * 6
    lib.inf_set_emu_keep.restype = _i
    lib.inf_set_emu_keep.argtypes = [_i, _i, _p, _p, _i, _p, _p, _p, _d, _p, _p]
    return lib


_emu = []


def emu():
    """tests/hostemu/informed_set_emu.cpp against csrc/informed_set_core.h, rebuilt when a source changes"""
    if not _emu:
        so = build_library(os.path.join(hostemu_lib.HOSTEMU, "libinformedsetemu.so"), hostemu_lib.sources([("informed_set_emu.cpp", [])]),
                           flags=hostemu_lib.FLAGS)
        _emu.append(declare(C.CDLL(so)))
    return _emu[0]


class EmuError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"{text} (status {status})")
        self.status = status


class EmuInformedSets:
    """``region_paths_sets`` and ``informed_regions_sets`` with the signatures of ``scene.DeviceScene`` through the host build, on
    geometry handed in.  ``order``: see ORDERS.  ``last``: the distances [B, P] the search left and the rounds of the last call"""

    def __init__(self, centers, lo, hi, row_ptr, tail, head, order=0, lib=None):
        self.lib = lib or emu()
        self.centers = np.ascontiguousarray(centers, float)
        self.P, self.n = self.centers.shape
        self.lo = None if lo is None else np.ascontiguousarray(lo, float)
        self.hi = None if hi is None else np.ascontiguousarray(hi, float)
        self.row_ptr, self.head = np.ascontiguousarray(row_ptr, np.int64), np.ascontiguousarray(head, np.int32)
        self.w = I.weights(self.centers, np.asarray(tail), self.head)
        self.order, self.last = order, None

    def check(self, rc):
        if rc:
            raise EmuError(rc, self.lib.inf_set_emu_last_error().decode())

    def _paths(self, B, lo, hi, ptr, reg, max_len, *rest):
        return self.lib.inf_set_emu_paths(self.P, self.n, self.row_ptr.ctypes.data, self.head.ctypes.data, self.w.ctypes.data, self.centers.ctypes.data, B,
                                          lo, hi, ptr, reg, max_len, self.order, *rest)

    def raw_paths(self, B, lo, hi, ptr, reg, max_len, *outs):
        a = lambda x: None if x is None else x.ctypes.data
        return self._paths(B, a(lo), a(hi), a(ptr), a(reg), max_len, *(a(o) for o in outs), None, None)

    def region_paths_sets(self, lo, hi, term_ptr, term_region, max_len=None):
        def call(B, lo, hi, ptr, reg, max_len, *outs):
            d, rounds = np.full((B, self.P), np.nan), np.zeros(B, np.int32)
            self.check(self._paths(B, lo, hi, ptr, reg, max_len, *outs, d.ctypes.data, rounds.ctypes.data))
            self.last = (d, rounds)
        return region_path_set_views(self.n, self.P, lo, hi, term_ptr, term_region, max_len, call)

    def raw_keep(self, B, lo, hi, bound, pad, keep):
        a = lambda x: None if x is None else x.ctypes.data
        return self.lib.inf_set_emu_keep(self.P, self.n, self.lo.ctypes.data, self.hi.ctypes.data, B, a(lo), a(hi), a(bound), pad, a(keep), None)

    def informed_regions_sets(self, lo, hi, bound, pad=SWEEP_PAD):
        call = lambda B, tlo, thi, bnd, pad, keep, num: self.check(
            self.lib.inf_set_emu_keep(self.P, self.n, self.lo.ctypes.data, self.hi.ctypes.data, B, tlo, thi, bnd, pad, keep, num))
        return informed_keep_set_array(self.n, self.P, lo, hi, bound, pad, call)


def emu_of(c, order=0, lib=None):
    return EmuInformedSets(c.centers, c.lo, c.hi, c.row_ptr, c.tail, c.head, order, lib)


def refusals(P, n, tlo, thi, term_ptr, term_region):
    """(label, text, kind, arguments) of every refusal of the two set calls: those of ``informed_cases.refusals`` with the boxes in the
    place of the points, and the ones the set calls add -- kind "paths" with dict(B, lo, hi, ptr, reg, max_len), kind "keep" with
    dict(B, lo, hi, bound, pad)"""
    B = len(tlo) // 2
    out = []
    for label, text, kind, a in I.refusals(P, n, tlo, term_ptr, term_region):
        a = dict(a)
        pts = a.pop("pts")
        a["lo"], a["hi"] = pts, (pts if pts is not tlo else thi)      # (a NaN coordinate: in both arrays)
        out.append((label, text.replace("NaN or negative", "not finite or negative"), kind, a))
    ok = dict(B=B, lo=tlo, hi=thi, ptr=term_ptr, reg=term_region, max_len=P)
    okk = dict(B=B, lo=tlo, hi=thi, bound=np.ones(B), pad=SWEEP_PAD)
    above = tlo.copy(); above[B, n - 1] = thi[B, n - 1] + 1e-9
    inf_hi = thi.copy(); inf_hi[1, 0] = np.inf
    inf_b = np.ones(B); inf_b[B - 1] = np.inf
    return out + [("null lo", "null", "paths", dict(ok, lo=None)), ("null hi", "null", "paths", dict(ok, hi=None)),
                  ("lo above hi", "lo above hi", "paths", dict(ok, lo=above)), ("inf side", "NaN or an inf", "paths", dict(ok, hi=inf_hi)),
                  ("null lo (keep)", "null", "keep", dict(okk, lo=None)), ("null hi (keep)", "null", "keep", dict(okk, hi=None)),
                  ("lo above hi (keep)", "lo above hi", "keep", dict(okk, lo=above)), ("inf side (keep)", "NaN or an inf", "keep", dict(okk, hi=inf_hi)),
                  ("inf bound", "not finite or negative", "keep", dict(okk, bound=inf_b))]
