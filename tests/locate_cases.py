"""Regions, points and checkers for the tests of locate_kernel (csrc/point_locate_core.h, csrc/polytope_lp.hip), shared by the host-build
tests (test_point_locate.py) and the device tests (test_gpu_point_locate.py), and the stand-in scene of the assembly tests.

Families: ``regions(kind, n, P, offset)`` -- ``"boxes"``; ``"polytopes"``: the box rows and random further rows, 2n .. 19 rows, the
count drawn per region (so it differs lane by lane); ``"scaled"``: those with every row multiplied by 10^u, u uniform(-3, 3) -- centres
uniform(0, 8) in the first min(n, 2) coordinates and uniform(-0.2, 0.2) in the rest, moved by ``offset`` (0 or 300), half-widths
uniform(0.05, 0.9).  ``points(...)``: even points uniform over the same domain, odd points around a region (centre + uniform(-1.3,
1.3) half-widths), so that a point lies in none to several regions.  The seeds are fixed.

The reference of the checkers is a ``numpy.longdouble`` restatement of g_i = a_i.p - b_i, s_i = sum |a_ik|, mag_i = sum |a_ik p_k| +
|b_i|; the kernel's own rule (2^-40 mag_i, eps + 2 tol) is NOT restated: the checks are the wider statements of soundness and
completeness, which any correct rule of that shape meets."""
from __future__ import annotations

import ctypes as C

import numpy as np

from hostemu_lib import emu_library


OUT, IN, UNDECIDED = 0, 1, 2
EPS, TOL = 1e-6, 1e-9
DIMS = (1, 2, 3, 8)
CHUNK = 256                              # LOCATE_CHUNK of point_locate_core.h (test_point_locate.py holds the two equal)
SIZES = (1, 63, 64, 65, 130, 600, 1000)  # one region; a stride less one, a stride, a stride and one; two strides and a tail; THREE
#                                          chunks with a partial last one (600 = 2 * 256 + 88); four chunks
QUERIES = (1, 2, 5, 130)
KINDS = ("boxes", "polytopes", "scaled")
OFFSETS = (0.0, 300.0)
FAMILIES = [(k, o) for k in KINDS for o in OFFSETS]


def _seed(kind, n, P, offset):
    return 100000 * KINDS.index(kind) + 10000 * n + 2 * P + (1 if offset else 0)


def _layout(rng, n, P, offset):
    c = rng.uniform(-0.2, 0.2, (P, n))
    c[:, :min(n, 2)] = rng.uniform(0, 8, (P, min(n, 2)))
    return c + offset, rng.uniform(0.05, 0.9, (P, n))


def regions(kind, n, P, offset=0.0):
    """list of (A, b)"""
    rng = np.random.default_rng(_seed(kind, n, P, offset))
    c, w = _layout(rng, n, P, offset)
    I = np.vstack([np.eye(n), -np.eye(n)])
    polys = []
    for p in range(P):
        A, b = I, np.hstack([c[p] + w[p], -(c[p] - w[p])])
        if kind != "boxes":
            extra = int(rng.integers(0, 19 - 2 * n + 1))
            d = rng.normal(size=(extra, n))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            A = np.vstack([A, d]); b = np.hstack([b, d @ c[p] + rng.uniform(0.05, 0.9, extra)])
        if kind == "scaled":
            f = 10.0 ** rng.uniform(-3, 3, len(b))
            A, b = A * f[:, None], b * f
        polys.append((np.ascontiguousarray(A), np.ascontiguousarray(b)))
    return polys


def points(kind, n, P, offset=0.0, Q=max(QUERIES)):
    """[Q, n]; the points of a smaller Q are the first Q of these"""
    rng = np.random.default_rng(_seed(kind, n, P, offset))
    c, w = _layout(rng, n, P, offset)            # the regions' own centres and half-widths (same seed, same draws)
    rng = np.random.default_rng(_seed(kind, n, P, offset) + 7)
    pts = rng.uniform(-0.3, 0.3, (Q, n)) + offset
    pts[:, :min(n, 2)] = rng.uniform(0, 8, (Q, min(n, 2))) + offset
    r = rng.integers(0, P, Q)
    near = c[r] + rng.uniform(-1.3, 1.3, (Q, n)) * w[r]
    pts[1::2] = near[1::2]
    return np.ascontiguousarray(pts)


def csr(polys, n):
    ptr = np.zeros(len(polys) + 1, np.int32)
    ptr[1:] = np.cumsum([len(b) for _, b in polys])
    A = np.ascontiguousarray(np.vstack([np.asarray(A, float).reshape(-1, n) for A, _ in polys])) if polys else np.zeros((0, n))
    b = np.ascontiguousarray(np.hstack([np.asarray(b, float).ravel() for _, b in polys])) if polys else np.zeros(0)
    return ptr, A, b


# ------------------------------------------------------------------------------------------- the extended-precision restatement
def exact_rows(polys, pts):
    """(g [Q, rows], s [rows], mag [Q, rows], ptr) in numpy.longdouble"""
    n = pts.shape[1]
    ptr, A, b = csr(polys, n)
    L = np.longdouble
    Al, bl, pl = A.astype(L), b.astype(L), pts.astype(L)
    g = np.zeros((len(pts), len(b)), L); mag = np.zeros_like(g)
    for k in range(n):
        g += pl[:, k:k + 1] * Al[None, :, k]
        mag += np.abs(pl[:, k:k + 1]) * np.abs(Al[None, :, k])
    return g - bl, np.abs(Al).sum(axis=1), mag + np.abs(bl), ptr


def _every(rows, ptr):
    return np.logical_and.reduceat(rows, ptr[:-1], axis=1)


def _some(rows, ptr):
    return np.logical_or.reduceat(rows, ptr[:-1], axis=1)


def dense(hits, Q, P):
    """class matrix [Q, P] (0: not listed) of a hit list, after checking the list's own consistency: int64 ``hit_ptr`` from 0 to the
    length, monotone; int32 regions in range, strictly ascending inside a point; classes 1 or 2"""
    hit_ptr, hit_region, hit_class = hits
    assert hit_ptr.dtype == np.int64 and hit_region.dtype == np.int32 and hit_class.dtype == np.uint8
    assert hit_ptr.shape == (Q + 1,) and hit_ptr[0] == 0 and hit_ptr[-1] == len(hit_region) == len(hit_class)
    assert np.all(np.diff(hit_ptr) >= 0)
    point_of = np.repeat(np.arange(Q, dtype=np.int64), np.diff(hit_ptr))
    assert np.all((hit_region >= 0) & (hit_region < max(P, 1))) and np.all((hit_class == IN) | (hit_class == UNDECIDED))
    assert np.all(np.diff(point_of * max(P, 1) + hit_region) > 0), "not ordered by point, then region index"
    M = np.zeros((Q, P), np.uint8)
    M[point_of, hit_region] = hit_class
    return M


def check_hits(hits, polys, pts, eps=EPS):
    """soundness and completeness of a hit list against the restatement; returns the number of UNDECIDED hits"""
    Q, P = len(pts), len(polys)
    M = dense(hits, Q, P)
    if Q == 0 or P == 0:
        return 0
    g, s, mag, ptr = exact_rows(polys, pts)
    # soundness: IN means p is in the region; not listed means some row keeps the whole eps-box out
    assert not np.any((M == IN) & ~_every(g <= 0, ptr))
    assert not np.any((M == OUT) & ~_some(g - np.longdouble(eps) * s > 0, ptr))
    # completeness: a point inside by a relative 1e-9 is IN; a row violated by 2.5 eps is absent (g > 0 follows from the bound for
    # every row but a row of zeros with b = 0, where g = s = 0 and nothing is violated)
    assert np.all(M[_every(g <= -np.longdouble(1e-9) * mag, ptr)] == IN)
    assert np.all(M[_some((g >= np.longdouble(2.5e-6) * s) & (g > 0), ptr)] == OUT)
    return int((M == UNDECIDED).sum())


# ------------------------------------------------------------------------------------------- crafted cases (n = 2)
def _box(lo, hi):
    return np.vstack([np.eye(2), -np.eye(2)]), np.array([hi[0], hi[1], -lo[0], -lo[1]], float)


WEDGE = (np.array([[-0.1, 1.0], [-0.1, -1.0], [1.0, 0.0]]), np.array([0.0, 0.0, 1.0]))      # y <= 0.1 x, -y <= 0.1 x, x <= 1


def crafted(zero_rows=True):
    """(names, polys, points, expect): ``expect[(point index, region name)]`` is the class the kernel must report.  ``zero_rows``:
    with the three regions that carry a row of zeros (the host build takes them; gcsadmm_scene_create refuses a zero facet normal)."""
    unit = _box((0, 0), (1, 1))
    with_row = lambda b0: (np.vstack([unit[0], np.zeros((1, 2))]), np.hstack([unit[1], [b0]]))
    regs = {"unit": unit, "wedge": WEDGE, "around": _box((-1e3, -1e3), (1e3, 1e3)), "sym": _box((-1, -1), (1, 1)), "far": _box((50, 50), (51, 51))}
    if zero_rows:
        regs.update(zero_pos=with_row(0.5), zero_null=with_row(0.0), zero_neg=with_row(-1.0))
    pts = np.array([[1.0, 0.5],                       # 0 exactly on a facet of unit
                    [1.0 + 0.5e-6, 0.5],              # 1 half an eps outside it
                    [1.0 + 3e-6, 0.5],                # 2 three eps outside
                    [1.0 + 0.9e-6, 1.0 + 0.9e-6],     # 3 on the diagonal off the corner: the box still reaches it
                    [-5e-6, 0.0],                     # 4 just beyond the wedge's acute vertex
                    [-0.0, -0.0],                     # 5 negative zeros: the centre of sym, and a corner of unit where every term
                    [0.0, 0.0],                       # 6 ... and the same point       of g and of r is zero, so the rows hold exactly: IN
                    [0.5, 0.5]])                      # 7 deep inside unit
    expect = {(0, "unit"): UNDECIDED, (1, "unit"): UNDECIDED, (2, "unit"): OUT, (3, "unit"): UNDECIDED, (4, "wedge"): UNDECIDED,
              (5, "sym"): IN, (6, "sym"): IN, (5, "unit"): IN, (6, "unit"): IN, (7, "unit"): IN, (7, "sym"): IN, (7, "wedge"): OUT}
    expect.update({(q, "around"): IN for q in range(len(pts))})
    expect.update({(q, "far"): OUT for q in range(len(pts))})
    if zero_rows:
        expect.update({(7, "zero_pos"): IN, (7, "zero_null"): IN, (7, "zero_neg"): OUT, (0, "zero_pos"): UNDECIDED, (0, "zero_neg"): OUT})
    return list(regs), list(regs.values()), pts, expect


def check_crafted(hits, names, polys, pts, expect):
    M = dense(hits, len(pts), len(polys))
    for (q, name), cls in expect.items():
        assert M[q, names.index(name)] == cls, (q, name, int(M[q, names.index(name)]), cls)
    assert np.array_equal(M[5], M[6]), "-0.0 and +0.0 classify differently"
    check_hits(hits, polys, pts)


# ------------------------------------------------------------------------------------------- the host build
def load_locate_emu():
    """tests/hostemu/locate_emu.cpp against csrc/point_locate_core.h, rebuilt when a source changes.  -ffp-contract=off:
    only the written fma calls fuse, as in the kernel"""
    lib = emu_library("locateemu")
    lib.locate_emu_hits.restype = C.c_longlong
    lib.locate_emu_hits.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    lib.locate_emu_scan.restype = C.c_int
    lib.locate_emu_scan.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.locate_emu_chunk.restype = C.c_int
    return lib


_emu = []


def emu():
    if not _emu:
        _emu.append(load_locate_emu())
    return _emu[0]


def emu_locate(polys, pts, eps=EPS, tol=TOL, n=None, lib=None):
    """(hit_ptr, hit_region, hit_class) of the host build: the count first, then the list -- the contract of ``DeviceScene.locate``"""
    lib = lib or emu()
    pts = np.ascontiguousarray(pts, float)
    n = n if n is not None else pts.shape[1]
    pts = pts.reshape(-1, n)
    ptr, A, b = csr(polys, n)
    Q, P = len(pts), len(polys)
    hit_ptr = np.zeros(Q + 1, np.int64)
    args = (n, P, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, Q, pts.ctypes.data, eps, tol, hit_ptr.ctypes.data)
    T = lib.locate_emu_hits(*args, None, None, -1)
    assert T >= 0, T
    hit_region = np.empty(T, np.int32); hit_class = np.empty(T, np.uint8)
    assert lib.locate_emu_hits(*args, hit_region.ctypes.data, hit_class.ctypes.data, T) == T
    return hit_ptr, hit_region, hit_class


_cache = {}


def family_hits(kind, n, P, offset, Q):
    """the host build's list for one family member, computed once (the device tests compare with it)"""
    key = (kind, n, P, offset, Q)
    if key not in _cache:
        _cache[key] = emu_locate(regions(kind, n, P, offset), points(kind, n, P, offset)[:Q])
    return _cache[key]


# ------------------------------------------------------------------------------------------- a stand-in scene for the assembly tests
class EmuScene:
    """The interface of ``scene.DeviceScene`` that ``SceneQueries`` uses, without a device: the region graph from a given list of
    overlapping region pairs (a committed edge list), the centres from ``graph.chebyshev_center``, ``locate`` from the host build."""

    def __init__(self, polys, pairs):
        self.polys, self.n = polys, polys[0][0].shape[1]
        pairs = sorted({(min(a, b), max(a, b)) for a, b in pairs})
        self.pa = np.array([a for a, _ in pairs], np.int32); self.pb = np.array([b for _, b in pairs], np.int32)
        self.locate_calls, self.closed = 0, False

    def centers(self):
        from gcs_admm_amd.graph import chebyshev_center
        P = len(self.polys)
        return np.stack([chebyshev_center(A, b) for A, b in self.polys]), np.ones(P), np.zeros(P, np.int32)

    def bounds(self):
        P = len(self.polys)
        return None, None, np.zeros((P, 2 * self.n), np.int32)

    def candidate_pairs(self):
        return len(self.pa)

    def overlaps(self, tol):
        return len(self.pa), 0

    def pairs(self):
        return self.pa, self.pb, np.ones(len(self.pa), np.uint8), np.zeros(len(self.pa), np.int32)

    def locate(self, pts, eps=EPS, tol=TOL):
        self.locate_calls += 1
        return emu_locate(self.polys, pts, eps, tol, n=self.n)

    def close(self):
        self.closed = True


class PairLP:
    """stand-in for the pair LPs of ``PolytopeScene.overlaps``, decided by ``graph.polytopes_overlap``; records its calls.  ``fail``:
    every LP reports status -1 with the wrong flag"""

    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def __call__(self, polys, pa, pb, tol, centers):
        from gcs_admm_amd.graph import polytopes_overlap
        self.calls.append((polys, np.array(pa), np.array(pb), tol, np.array(centers)))
        flags = np.array([1 if polytopes_overlap(*polys[a], *polys[b]) else 0 for a, b in zip(pa, pb)], np.uint8)
        st = np.zeros(len(pa), np.int32)
        if self.fail:
            st[:] = -1; flags = 1 - flags
        return flags, st


def region_sets(name):
    """(As, bs, n, region pairs) of a scene for ``SceneQueries``: ``"four_boxes"`` (scene_fakes.py) or the regions of a committed
    benchmark with the region-region part of its committed edge list"""
    if name == "four_boxes":
        from scene_fakes import four_boxes
        As, bs = four_boxes()
        return As, bs, 2, [(0, 1), (1, 2)]
    from gcs_admm_amd.cases import fixture_sets, load_fixture
    As, bs, n, _, _ = fixture_sets(name)
    case = load_fixture(name)[0]
    keys = [k for k in As if k not in ('s', 't')]
    pairs = [(keys.index(u), keys.index(w)) for u, w in case["edges"] if u not in ('s', 't') and w not in ('s', 't')]
    return {k: As[k] for k in keys}, {k: bs[k] for k in keys}, n, pairs
