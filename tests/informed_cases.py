"""Scenes, queries, the host build and a plain-numpy restatement for the tests of the informed region set (csrc/informed_core.h;
gcsadmm_scene_region_paths / _informed_regions in csrc/polytope_lp.hip), shared by test_informed.py (host build, no GPU) and
test_gpu_informed.py.

The restatement is written from the rule, not from the header: a heap Dijkstra on the region graph with the same weight, the same goal
choice and the same tie rules, and the keep rule.  Both are monotone in floating point (a + w does not fall when a does not), so
Dijkstra's distances are the fixed point the kernel's rounds reach, up to the rounding of the weights: the compiler may contract the
sums of the device build, so costs are compared within ``margin`` and bits only where every sum is exact (``integer_lattice``)."""
from __future__ import annotations

import ctypes as C
import heapq
import os

import numpy as np

import sweep_cases as S
from hostemu_lib import emu_library
from gcs_admm_amd.scene import SWEEP_PAD, candidate_pairs, edge_arrays, informed_keep_array, region_path_views

ROOT = S.ROOT
EMU_SRC = os.path.join(ROOT, "tests", "hostemu", "informed_emu.cpp")
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2
EPS = 1e-6
SLACK = 1e-9          # the keep rule's relative widening of the bound
NEAR = 1e-12          # a flag may differ from the restatement's only where lb is this close (relative to the bound) to the threshold
BATCHES = (1, 2, 3, 4, 5)


def margin(length, n):
    """relative: above the rounding of two polyline costs over ``length`` regions in dimension n.  With u = 2^-53: a distance is off by
    at most (n / 2 + 1) u (n squares summed, halved by the root, the root itself; a contracted sum is no worse), the length adds of a
    cost by u each, so two costs differ by at most 2 (length + n / 2 + 1) u = (length + n / 2 + 1) 2^-52"""
    return (length + n + 4) * 2.0 ** -52


# ------------------------------------------------------------------------------------------- scenes of boxes
def box_polys(lo, hi):
    n = lo.shape[1]
    A = np.vstack([np.eye(n), -np.eye(n)])
    return [(A.copy(), np.hstack([h, -l])) for l, h in zip(lo, hi)]


def _lattice(wall):
    from gcs_admm_amd.graph import lattice_boxes
    g = lattice_boxes(6, 8)
    lo, hi = [], []
    for v in range(2, g.num_vertices):
        A, b = g.poly_A[g.poly_ptr[v]:g.poly_ptr[v + 1]], g.poly_b[g.poly_ptr[v]:g.poly_ptr[v + 1]]
        hi.append([min(b[i] / A[i, k] for i in range(len(b)) if A[i, k] > 0) for k in range(2)])
        lo.append([max(b[i] / A[i, k] for i in range(len(b)) if A[i, k] < 0) for k in range(2)])
    lo, hi = np.array(lo), np.array(hi)
    if wall:      # row 4 without its last cell: every path from below to above goes round the right end
        stays = np.ones(48, bool)
        stays[4 * 6:4 * 6 + 5] = False
        lo, hi = lo[stays], hi[stays]
    return lo, hi


def _random_boxes(n, P, extent, seed):
    rng = np.random.default_rng(seed)
    cen = rng.uniform(0.0, 1.0, (P, n)) * np.asarray(extent, float)
    half = rng.uniform(0.45, 0.95, (P, n))
    return cen - half, cen + half


def scene_boxes(name):
    """(lo, hi) [P, n] of a named scene: ``lattice`` (the cells of graph.lattice_boxes(6, 8)), ``lattice_wall`` (without a wall of five),
    ``lattice_twice`` (every cell a second time behind the 48: region r + 48 has the polytope, the centre and the neighbours of r, at
    distance 0 from it, so every distance ties exactly whatever the centres are),
    ``boxes2`` / ``boxes3`` (60 random overlapping boxes at n = 2 / 3), ``boxes300`` (300 at n = 2: a lane of the path kernel owns two
    vertices, and a launch has several rounds), ``islands`` (two components), ``single`` (start and goal share one region)"""
    if name in ("lattice", "lattice_wall"):
        return _lattice(name == "lattice_wall")
    if name == "lattice_twice":
        lo, hi = _lattice(False)
        return np.vstack([lo, lo]), np.vstack([hi, hi])
    if name == "boxes2":
        return _random_boxes(2, 60, (9.0, 7.0), 11)
    if name == "boxes3":
        return _random_boxes(3, 60, (4.0, 4.0, 3.0), 12)
    if name == "boxes300":
        return _random_boxes(2, 300, (40.0, 8.0), 13)
    if name == "islands":
        lo_a, hi_a = _random_boxes(2, 12, (3.0, 3.0), 14)
        lo_b, hi_b = _random_boxes(2, 12, (3.0, 3.0), 15)
        return np.vstack([lo_a, lo_b + 20.0]), np.vstack([hi_a, hi_b + 20.0])
    assert name == "single", name
    return _random_boxes(2, 8, (3.0, 3.0), 16)


SCENES = ("lattice", "lattice_wall", "lattice_twice", "boxes2", "boxes3", "boxes300", "islands", "single")


def region_graph_of(lo, hi):
    """(row_ptr int64 [P + 1], tail, head int32) of the boxes that overlap (closed sets), the arrays of DeviceScene.region_graph"""
    pa, pb = candidate_pairs(lo, hi, 0.0)
    tail, head = edge_arrays(pa, pb, np.ones(len(pa), np.uint8))
    row_ptr = np.zeros(len(lo) + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(tail, minlength=len(lo)))
    return row_ptr, tail, head


def components(P, tail, head):
    label = np.arange(P)
    while True:
        low = label.copy()
        np.minimum.at(low, tail, label[head])
        if np.array_equal(low, label):
            return label
        label = low


def queries(name, lo, hi, tail, head):
    """five queries (S [5, n], G [5, n]) of a scene, points strictly inside regions: 0, 1 local (goal in a neighbour of a neighbour), 2
    across the scene, 3, 4 random pairs; ``islands``: 0, 1 across the two components; ``single``: both points in one region"""
    P, n = lo.shape
    rng = np.random.default_rng(100 + P)
    inside = lambda r: lo[r] + rng.uniform(0.3, 0.7, n) * (hi[r] - lo[r])
    if name == "single":
        rs = rng.integers(0, P, 5)
        return np.array([inside(r) for r in rs]), np.array([inside(r) for r in rs])
    mid = 0.5 * (lo + hi)
    label = components(P, tail, head)
    big = np.nonzero(label == np.bincount(label).argmax())[0]
    near = lambda r: big[np.argsort(np.linalg.norm(mid[big] - mid[r], axis=1))[min(6, len(big) - 1)]]
    a, b = big[rng.integers(0, len(big), 4)], big[rng.integers(0, len(big), 4)]
    far = (big[np.argmin(mid[big, 0])], big[np.argmax(mid[big, 0])])
    pairs = [(a[0], near(a[0])), (a[1], near(a[1])), far, (a[2], b[2]), (a[3], b[3])]
    if name == "islands":
        other = np.nonzero(label != label[big[0]])[0]
        pairs[0], pairs[1] = (big[0], other[0]), (other[-1], big[-1])
    return np.array([inside(r) for r, _ in pairs]), np.array([inside(r) for _, r in pairs])


def regions_under(lo, hi, pts, eps=EPS):
    """the ascending int32 list of the boxes that meet ``[p - eps, p + eps]``, per point"""
    return [np.nonzero(np.all((lo <= p + eps) & (p - eps <= hi), axis=1))[0].astype(np.int32) for p in pts]


def term_lists(regs):
    term_ptr = np.zeros(len(regs) + 1, np.int64)
    term_ptr[1:] = np.cumsum([len(r) for r in regs])
    return term_ptr, (np.concatenate(regs).astype(np.int32) if regs else np.zeros(0, np.int32))


class Case:
    """a named scene with its nominal geometry (centres: the middles of the boxes), its region graph and its five queries"""

    def __init__(self, name):
        self.name = name
        self.lo, self.hi = scene_boxes(name)
        self.P, self.n = self.lo.shape
        self.centers = np.ascontiguousarray(0.5 * (self.lo + self.hi))
        self.row_ptr, self.tail, self.head = region_graph_of(self.lo, self.hi)
        # (lattice_twice: the points of the lattice, each under a cell and its copy)
        self.S, self.G = (case("lattice").S, case("lattice").G) if name == "lattice_twice" else queries(name, self.lo, self.hi, self.tail, self.head)
        self.polys = box_polys(self.lo, self.hi)

    def batch(self, B):
        """(points [2 B, n], term_ptr, term_region) of the first B queries"""
        pts = np.ascontiguousarray(np.vstack([self.S[:B], self.G[:B]]))
        return (pts,) + term_lists(regions_under(self.lo, self.hi, pts))


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def integer_lattice(nx=9, ny=7):
    """(centres [P, 2] of integers, row_ptr, tail, head of the 4-neighbour grid, points [10, 2], term_ptr, term_region): every weight
    is 1 and every point an integer point, so every sum is exact and most shortest paths tie.  Query 1 starts under two regions."""
    P = nx * ny
    idx = lambda i, j: j * nx + i
    cen = np.array([[i, j] for j in range(ny) for i in range(nx)], float)
    pairs = [(idx(i, j), idx(i + 1, j)) for j in range(ny) for i in range(nx - 1)] + [(idx(i, j), idx(i, j + 1)) for j in range(ny - 1) for i in range(nx)]
    pa, pb = np.array(pairs, np.int32).T
    tail, head = edge_arrays(pa, pb, np.ones(len(pa), np.uint8))
    row_ptr = np.zeros(P + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(tail, minlength=P))
    starts = [(0, 0), (1, 1), (8, 0), (4, 3), (2, 6)]
    goals = [(8, 6), (7, 5), (0, 6), (4, 3), (6, 1)]
    regs = [[idx(*p)] for p in starts] + [[idx(*p)] for p in goals]
    regs[1] = sorted([idx(1, 1), idx(2, 1)])
    regs[5 + 1] = sorted([idx(7, 5), idx(7, 4), idx(6, 5)])
    return cen, row_ptr, tail, head, np.array(starts + goals, float), *term_lists([np.array(r, np.int32) for r in regs])


# ------------------------------------------------------------------------------------------- the restatement
def weights(centers, tail, head):
    diff = centers[tail] - centers[head]
    sq = np.zeros(len(tail))
    for k in range(centers.shape[1]):      # ascending coordinate order
        sq = sq + diff[:, k] * diff[:, k]
    return np.sqrt(sq)


def dist(a, b):
    sq = 0.0
    for k in range(len(a)):
        sq = sq + (a[k] - b[k]) * (a[k] - b[k])
    return float(np.sqrt(sq))


def restate_path(centers, row_ptr, head, w, s, g, rs, rt, max_len=None):
    """(path, cost, status, d) of one query by the rule: heap Dijkstra from init, the goal choice, the backtrack"""
    P = len(row_ptr) - 1
    max_len = P if max_len is None else max_len
    init = np.full(P, np.inf)
    for r in rs:
        init[r] = dist(s, centers[r])
    d = init.copy()
    heap = [(d[r], int(r)) for r in rs]
    heapq.heapify(heap)
    done = np.zeros(P, bool)
    while heap:
        du, u = heapq.heappop(heap)
        if done[u] or du > d[u]:
            continue
        done[u] = True
        for p in range(row_ptr[u], row_ptr[u + 1]):      # (symmetric graph: the row of u lists its out-neighbours too, same weights)
            v = head[p]
            if du + w[p] < d[v]:
                d[v] = du + w[p]
                heapq.heappush(heap, (d[v], int(v)))
    cost, goal = np.inf, -1
    for r in rt:
        c = d[r] + dist(centers[r], g)
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


def polyline_cost(centers, s, g, path):
    total = dist(s, centers[path[0]])
    for u, v in zip(path[:-1], path[1:]):
        total = total + dist(centers[u], centers[v])
    return total + dist(centers[path[-1]], g)


def box_distance(p, lo, hi, pad):
    t = np.maximum(np.maximum(lo - pad - p, 0.0), p - hi - pad)
    sq = np.zeros(len(lo))
    for k in range(lo.shape[1]):
        sq = sq + t[:, k] * t[:, k]
    return np.sqrt(sq)


def restate_keep(lo, hi, s, g, bound, pad=SWEEP_PAD):
    """(keep bool [P], near bool [P]: lb within NEAR * bound of the threshold, where a build may decide either way)"""
    lb = box_distance(s, lo, hi, pad) + box_distance(g, lo, hi, pad)
    limit = bound * (1.0 + SLACK)
    with np.errstate(invalid="ignore"):
        near = np.abs(lb - limit) <= NEAR * bound if np.isfinite(bound) else np.zeros(len(lo), bool)
    return lb <= limit, near


def check_paths(got, centers, row_ptr, tail, head, w, pts, term_ptr, term_region, exact=False):
    """``got = (paths, cost, status)`` of B queries against the rule and the restatement; returns the restatement's results.  ``exact``:
    ``"paths"`` the paths equal the restatement's vertex for vertex, ``True`` the costs bit for bit too"""
    paths, cost, status = got
    B = len(status)
    edges = set(zip(tail.tolist(), head.tolist()))
    n = centers.shape[1]
    ref = []
    for i in range(B):
        rs, rt = term_region[term_ptr[i]:term_ptr[i + 1]], term_region[term_ptr[B + i]:term_ptr[B + i + 1]]
        want = restate_path(centers, row_ptr, head, w, pts[i], pts[B + i], rs, rt)
        ref.append(want)
        assert status[i] == want[2], (i, status[i], want[2])
        if want[2] != 0:
            assert len(paths[i]) == 0 and cost[i] == np.inf
            continue
        p = paths[i]
        assert p.dtype == np.int32 and len(p) >= 1 and p[0] in rs and p[-1] in rt, (i, p)
        assert all((int(u), int(v)) in edges for u, v in zip(p[:-1], p[1:])), (i, p)
        tol = margin(len(p), n)
        assert abs(cost[i] - polyline_cost(centers, pts[i], pts[B + i], p)) <= tol * cost[i], i
        assert abs(cost[i] - want[1]) <= tol * want[1], (i, cost[i], want[1])
        if exact:
            assert np.array_equal(p, want[0]), (i, p, want[0])
        if exact is True:
            assert cost[i] == want[1], (i, cost[i], want[1])
    return ref


def check_keep(got, lo, hi, pts, bound, pad=SWEEP_PAD):
    """bool [B, P] against the restatement; no region of these cases may be near the threshold"""
    B = len(bound)
    assert got.dtype == bool and got.shape == (B, len(lo))
    for i in range(B):
        want, near = restate_keep(lo, hi, pts[i], pts[B + i], bound[i], pad)
        assert not near.any(), (i, np.nonzero(near)[0])
        assert np.array_equal(got[i], want), (i, np.nonzero(got[i] != want)[0])


# ------------------------------------------------------------------------------------------- the host build
_p, _i, _d, _ll = C.c_void_p, C.c_int, C.c_double, C.c_longlong


def declare(lib):
    lib.inf_emu_last_error.restype = C.c_char_p
    lib.inf_emu_last_error.argtypes = []
    lib.inf_emu_chunk.restype = _i
    lib.inf_emu_chunk.argtypes = [_i]
    lib.inf_emu_weights.restype = None
    lib.inf_emu_weights.argtypes = [_i, _p, _ll, _p, _p, _p]
    lib.inf_emu_paths.restype = _i
    lib.inf_emu_paths.argtypes = [_i, _i, _p, _p, _p, _p, _i, _p, _p, _p, _i, _i] + [_p] * 6
    lib.inf_emu_keep.restype = _i
    lib.inf_emu_keep.argtypes = [_i, _i, _p, _p, _i, _p, _p, _d, _p, _p]
    return lib


def load_informed_emu():
    """tests/hostemu/informed_emu.cpp against csrc/informed_core.h, rebuilt when a source changes"""
    return declare(emu_library("informedemu"))


_emu = []


def emu():
    if not _emu:
        _emu.append(load_informed_emu())
    return _emu[0]


class EmuError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"{text} (status {status})")
        self.status = status


class EmuInformed:
    """``region_paths`` and ``informed_regions`` with the signatures of ``scene.DeviceScene`` through the host build, on geometry handed
    in.  ``order``: 0 the lanes of a round forwards, 1 backwards.  ``last``: the settled distances [B, P] and the rounds of the last call"""

    def __init__(self, centers, lo, hi, row_ptr, tail, head, order=0, lib=None):
        self.lib = lib or emu()
        self.centers = np.ascontiguousarray(centers, float)
        self.P, self.n = self.centers.shape
        self.lo = None if lo is None else np.ascontiguousarray(lo, float)
        self.hi = None if hi is None else np.ascontiguousarray(hi, float)
        self.row_ptr, self.tail, self.head = np.ascontiguousarray(row_ptr, np.int64), np.ascontiguousarray(tail, np.int32), np.ascontiguousarray(head, np.int32)
        self.w = np.empty(len(self.tail))
        self.lib.inf_emu_weights(self.n, self.centers.ctypes.data, len(self.tail), self.tail.ctypes.data, self.head.ctypes.data, self.w.ctypes.data)
        self.order, self.last = order, None

    def check(self, rc):
        if rc:
            raise EmuError(rc, self.lib.inf_emu_last_error().decode())

    def raw_paths(self, B, pts, ptr, reg, max_len, *outs):
        a = lambda x: None if x is None else x.ctypes.data
        return self.lib.inf_emu_paths(self.P, self.n, self.row_ptr.ctypes.data, self.head.ctypes.data, self.w.ctypes.data, self.centers.ctypes.data, B, a(pts),
                                      a(ptr), a(reg), max_len, self.order, *(a(o) for o in outs), None, None)

    def region_paths(self, points, term_ptr, term_region, max_len=None):
        def call(B, pts, ptr, reg, max_len, *outs):
            d, rounds = np.full((B, self.P), np.nan), np.zeros(B, np.int32)
            self.check(self.lib.inf_emu_paths(self.P, self.n, self.row_ptr.ctypes.data, self.head.ctypes.data, self.w.ctypes.data, self.centers.ctypes.data, B,
                                              pts, ptr, reg, max_len, self.order, *outs, d.ctypes.data, rounds.ctypes.data))
            self.last = (d, rounds)
        return region_path_views(self.n, self.P, points, term_ptr, term_region, max_len, call)

    def raw_keep(self, B, pts, bound, pad, keep):
        a = lambda x: None if x is None else x.ctypes.data
        return self.lib.inf_emu_keep(self.P, self.n, self.lo.ctypes.data, self.hi.ctypes.data, B, a(pts), a(bound), pad, a(keep), None)

    def informed_regions(self, points, bound, pad=SWEEP_PAD):
        call = lambda B, pts, bnd, pad, keep, num: self.check(self.lib.inf_emu_keep(self.P, self.n, self.lo.ctypes.data, self.hi.ctypes.data, B, pts, bnd, pad, keep, num))
        return informed_keep_array(self.n, self.P, points, bound, pad, call)


def emu_of(c, order=0, lib=None):
    return EmuInformed(c.centers, c.lo, c.hi, c.row_ptr, c.tail, c.head, order, lib)


def refusals(P, n, pts, term_ptr, term_region):
    """(label, text, kind, arguments) of every refusal of the two calls, made from a valid call of B >= 2 queries whose first list has
    two regions or more: kind "paths" with dict(B, pts, ptr, reg, max_len), kind "keep" with dict(B, pts, bound, pad)"""
    B = len(pts) // 2
    assert B >= 2 and term_ptr[1] >= 2
    ok = dict(B=B, pts=pts, ptr=term_ptr, reg=term_region, max_len=P)
    okk = dict(B=B, pts=pts, bound=np.ones(B), pad=SWEEP_PAD)
    twice = term_region.copy(); twice[1] = twice[0]
    swapped = term_region.copy(); swapped[[0, 1]] = swapped[[1, 0]]
    high = term_region.copy(); high[term_ptr[1] - 1] = P
    low = term_region.copy(); low[0] = -1
    down = term_ptr.copy(); down[1] = term_ptr[2] + 1
    nan_pt = pts.copy(); nan_pt[0, 0] = np.nan
    nan_b = np.ones(B); nan_b[1] = np.nan
    neg_b = np.ones(B); neg_b[0] = -1e-300
    return [("max_len = 0", "max_len", "paths", dict(ok, max_len=0)),
            ("negative num_queries", "negative", "paths", dict(ok, B=-1)),
            ("list with a repeat", "strictly ascending", "paths", dict(ok, reg=twice)),
            ("list descending", "strictly ascending", "paths", dict(ok, reg=swapped)),
            ("region = P", "out of range", "paths", dict(ok, reg=high)),
            ("region < 0", "out of range", "paths", dict(ok, reg=low)),
            ("term_ptr decreasing", "non-decreasing", "paths", dict(ok, ptr=down)),
            ("NaN point", "NaN or an inf", "paths", dict(ok, pts=nan_pt)),
            ("null term_ptr", "null", "paths", dict(ok, ptr=None)),
            ("NaN bound", "NaN or negative", "keep", dict(okk, bound=nan_b)),
            ("negative bound", "NaN or negative", "keep", dict(okk, bound=neg_b)),
            ("NaN pad", "pad is NaN", "keep", dict(okk, pad=float("nan"))),
            ("NaN point (keep)", "NaN or an inf", "keep", dict(okk, pts=nan_pt)),
            ("negative num_queries (keep)", "negative", "keep", dict(okk, B=-1))]
