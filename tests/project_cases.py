"""Radii, crafted cases, references and the host build for the tests of the projection kernels (csrc/point_project_core.h), shared by the
host-build tests (test_point_project.py) and the device tests (test_gpu_point_project.py).  The regions and points are those of
locate_cases.py, imported.

The reference of a pair is NOT the code under test: ``reference(A, b, p)`` solves the least-distance problem of Lawson and Hanson
(min |y| s.t. -A^ y >= A^ p - b^, a non-negative least-squares solve written out here), takes the rows that are tight at its answer and
carry a multiplier and solves the equality-constrained projection on them again in ``numpy.longdouble`` (a k x k elimination written out here), and checks the KKT conditions of what it
returns in longdouble: feasible, multipliers >= 0.  ``certificate`` is the duality certificate of the issue, from a second nnls on the
rows that are tight at the x under test."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
from scipy.optimize import nnls

import hostemu_lib
import locate_cases as lc
from gcs_admm_amd.native_build import build_library

L = np.longdouble
OUT, INSIDE, OUTSIDE = 0, 1, 2
SOLVED, BEYOND, FAILED = 0, 1, -1
RADII = (0.0, 0.05, 0.5, np.inf)
SIZES = (1, 65, 600)          # one region; a stride and one; three chunks of LOCATE_CHUNK = 256 with a partial last one
Q = 12
MAX_ITER = 100
ALLOW = L(2.0) ** -40         # the allowance of locate_classify


def radii(num):
    """the radii of ``num`` points: the cycle 0, 0.05, 0.5, inf"""
    return np.array([RADII[q % len(RADII)] for q in range(num)], float)


# ------------------------------------------------------------------------------------------- the reference
def normalised(A, b):
    """(A^, b^) in longdouble"""
    Al, bl = np.asarray(A, float).astype(L), np.asarray(b, float).astype(L)
    nrm = np.sqrt((Al * Al).sum(axis=1))
    return Al / nrm[:, None], bl / nrm


def _solve(M, y):
    """M x = y by elimination with partial pivoting, in the dtype of M (numpy.linalg has no longdouble)"""
    M, y = M.copy(), y.copy()
    k = len(y)
    for c in range(k):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        if piv != c:
            M[[c, piv]] = M[[piv, c]]; y[[c, piv]] = y[[piv, c]]
        for r in range(c + 1, k):
            f = M[r, c] / M[c, c]
            M[r, c:] -= f * M[c, c:]; y[r] -= f * y[c]
    x = np.zeros(k, M.dtype)
    for c in range(k - 1, -1, -1):
        x[c] = (y[c] - M[c, c + 1:] @ x[c + 1:]) / M[c, c]
    return x


def _nnls(E, f):
    """min |E u - f| over u >= 0 by the active-set method of Lawson and Hanson, written out (float64): the reference must not hang on
    one library routine, and whatever this returns is only a guess that ``reference`` verifies"""
    m = E.shape[1]
    passive, u = np.zeros(m, bool), np.zeros(m)
    for _ in range(10 * m):
        w = E.T @ (f - E @ u)
        w[passive] = -np.inf
        j = int(np.argmax(w))
        if not w[j] > 1e-13:
            break
        passive[j] = True
        for _ in range(10 * m):
            s = np.zeros(m)
            s[passive] = np.linalg.lstsq(E[:, passive], f, rcond=None)[0]
            if s[passive].min() > 0:
                break
            bad = passive & (s <= 0)
            alpha = (u[bad] / (u[bad] - s[bad])).min()
            u = u + alpha * (s - u)
            passive &= u > 1e-15
        u = s
    return u


def reference(A, b, p):
    """(x* longdouble [n], d* longdouble) of the projection of p onto {A x <= b}"""
    Ah, bh = normalised(A, b)
    pl = np.asarray(p, float).astype(L)
    g = Ah @ pl - bh
    if np.all(g <= 0):
        return pl, L(0)
    n = len(pl)
    # least-distance programming: y = x - p, G y >= h with G = -A^, h = g; u = nnls([G'; h'], e_n+1), r = E u - e_n+1, y = -r[:n] / r[n]
    E = np.vstack([-Ah.astype(float).T, g.astype(float)[None, :]])
    f = np.zeros(n + 1); f[n] = 1.0
    u = _nnls(E, f)
    r = E @ u - f
    assert r[n] < 0, "the region is empty"
    x0 = pl.astype(float) - r[:n] / r[n]
    # the rows that are tight there and carry a multiplier, and of those an independent set
    tight = bh - Ah @ x0.astype(L) <= L(1e-9) * max(1.0, np.abs(x0).max())
    keep = []
    for i in np.argsort(-u):
        if tight[i] and u[i] > 1e-9 * u.max():
            rows = Ah[keep + [int(i)]].astype(float)
            if np.linalg.matrix_rank(rows, tol=1e-9) == len(keep) + 1:
                keep.append(int(i))
    N = Ah[keep]
    mu = _solve(N @ N.T, g[keep])
    x = pl - N.T @ mu
    # the KKT conditions of what is returned, whatever the guesses above were: feasible, multipliers >= 0 (stationarity and
    # complementarity hold by construction)
    scale = np.abs(Ah) @ np.abs(x) + np.abs(bh)
    assert np.all(mu >= -L(1e-12) * max(L(1), np.abs(mu).max())), ("multipliers", mu)
    assert np.all(Ah @ x - bh <= L(1e-15) * scale), ("feasibility", float((Ah @ x - bh).max()))
    return x, np.sqrt(((x - pl) ** 2).sum())


def lower_bounds(polys, pts):
    """[Q, P] longdouble: max(0, max_i g_i) of every pair, the distance to the most violated half-space; 0 iff the point is inside"""
    n = pts.shape[1]
    ptr = np.concatenate([[0], np.cumsum([len(b) for _, b in polys])])
    Ah = np.vstack([normalised(A, b)[0] for A, b in polys]); bh = np.hstack([normalised(A, b)[1] for A, b in polys])
    g = pts.astype(L) @ Ah.T - bh
    return np.maximum(np.maximum.reduceat(g, ptr[:-1], axis=1), 0)


def reference_call(polys, pts, rad=None):
    """(X [Q, P, n], D [Q, P]) in longdouble.  With ``rad`` only the pairs that matter are solved: those whose lower bound is within
    rad (1 + 1e-6) (finite radii), and per point the regions in ascending order of their lower bounds until that exceeds the second
    smallest distance found (the two nearest regions).  Every other pair has D = +inf, which stands for "beyond the radius, and not one
    of the two nearest", and X = nan."""
    n = pts.shape[1]
    low = lower_bounds(polys, pts)
    X = np.full((len(pts), len(polys), n), np.nan, L); D = np.full((len(pts), len(polys)), np.inf, L)
    for q, p in enumerate(pts):
        best = []
        for r in np.argsort(low[q], kind="stable"):
            near = rad is None or (np.isfinite(rad[q]) and low[q, r] <= L(rad[q]) * (1 + L(1e-6)))
            if not near and len(best) >= 2 and low[q, r] > sorted(best)[1] * (1 + L(1e-6)):
                if not np.isfinite(rad[q]) or low[q, r] > L(rad[q]) * (1 + L(1e-6)):
                    break
                continue
            X[q, r], D[q, r] = reference(*polys[r], p)
            best.append(D[q, r])
    return X, D, low


def feasibility(A, b, x):
    """max_i (a_i.x - b_i) / (sum_k |a_ik x_k| + |b_i|) in longdouble: at most 2^-40 for a solved hit"""
    Al, bl, xl = np.asarray(A, float).astype(L), np.asarray(b, float).astype(L), np.asarray(x, float).astype(L)
    viol, scale = Al @ xl - bl, np.abs(Al) @ np.abs(xl) + np.abs(bl)
    zero = scale == 0                      # (a row through the origin at x = 0: satisfied exactly, or not at all)
    return np.where(zero, np.where(viol <= 0, L(0), L(np.inf)), viol / np.where(zero, L(1), scale)).max()


def certificate(A, b, p, x):
    """(gap, scale) of the issue's duality certificate, longdouble: lambda >= 0 from nnls over the normalised rows whose slack at x is
    below 1e-9 max(1, |x|_inf), q(lambda) = -1/2 |A^' lambda|^2 + lambda' (A^ p - b^), gap = 1/2 |x - p|^2 - q, to be held to
    1e-9 scale with scale = max(d^2, 2^-40 (|p|_inf + 1)^2)"""
    Ah, bh = normalised(A, b)
    pl, xl = np.asarray(p, float).astype(L), np.asarray(x, float).astype(L)
    tight = np.nonzero(bh - Ah @ xl < L(1e-9) * max(L(1), np.abs(xl).max()))[0]
    lam = np.zeros(len(bh), L)
    if len(tight):
        lam[tight] = nnls(Ah[tight].astype(float).T, (pl - xl).astype(float), maxiter=50 * len(tight))[0]
    v = Ah.T @ lam
    q = -L(0.5) * (v @ v) + lam @ (Ah @ pl - bh)
    d2 = ((xl - pl) ** 2).sum()
    return L(0.5) * d2 - q, max(d2, ALLOW * (np.abs(pl).max() + 1) ** 2)


# ------------------------------------------------------------------------------------------- crafted cases (n = 2)
def _box(lo, hi):
    return np.vstack([np.eye(2), -np.eye(2)]), np.array([hi[0], hi[1], -lo[0], -lo[1]], float)


def crafted():
    """(names, polys, points, radius, expect): n = 2.  ``expect[(point, region name)]`` is None (not listed) or (class, status, x, d,
    iterations or None)."""
    unit = _box((0, 0), (1, 1))
    repeated = (np.vstack([unit[0], unit[0][:1]]), np.hstack([unit[1], unit[1][:1]]))                # the row x <= 1 twice
    rescaled = (np.vstack([unit[0], 1e3 * unit[0][:1]]), np.hstack([unit[1], 1e3 * unit[1][:1]]))    # ... and at two scalings
    s = np.sqrt(0.5)
    corner = (np.vstack([unit[0], [[s, s]]]), np.hstack([unit[1], [2 * s]]))                         # x + y <= 2 through (1, 1)
    regs = {"unit": unit, "wedge": lc.WEDGE, "repeated": repeated, "rescaled": rescaled, "corner": corner,
            "left": _box((-3, 0), (-2, 1)), "right": _box((2, 0), (3, 1)), "far": _box((50, 50), (51, 51)),
            "diag": (np.array([[-s, -s], [1.0, 0.0], [0.0, 1.0]]), np.array([-20 * s, 30.0, 30.0]))}      # x + y >= 20
    pts = np.array([[0.5, 0.5],            # 0 inside unit
                    [1.0, 0.5],            # 1 exactly on a facet of unit: INSIDE, x = p
                    [1.0 + 1e-9, 0.5],     # 2 1e-9 beyond that facet
                    [1.5, 1.25],           # 3 beyond the vertex (1, 1): two active rows
                    [-1e-5, 0.0],          # 4 beyond the wedge's acute vertex: the apex, d = 1e-5
                    [0.0, 0.5],            # 5 on a facet of unit, 2 from `left` and 2 from `right`; `far` is beyond its radius 2.5
                    [8.0, 9.0]])           # 6 3 sqrt(1/2) from the half-plane of `diag`, within its radius 3; `far` is not
    rad = np.array([np.inf, np.inf, np.inf, np.inf, np.inf, 2.5, 3.0])
    hyp = float(np.hypot(0.5, 0.25))
    step = float(np.float64(1.0 + 1e-9) - 1.0)      # what 1 + 1e-9 is beyond 1 as a double
    expect = {(0, "unit"): (INSIDE, SOLVED, (0.5, 0.5), 0.0, 0), (1, "unit"): (INSIDE, SOLVED, (1.0, 0.5), 0.0, 0),
              (2, "unit"): (OUTSIDE, SOLVED, (1.0, 0.5), step, 1), (3, "unit"): (OUTSIDE, SOLVED, (1.0, 1.0), hyp, 2),
              (4, "wedge"): (OUTSIDE, SOLVED, (0.0, 0.0), 1e-5, None),
              (3, "repeated"): (OUTSIDE, SOLVED, (1.0, 1.0), hyp, 2), (3, "rescaled"): (OUTSIDE, SOLVED, (1.0, 1.0), hyp, 2),
              (3, "corner"): (OUTSIDE, SOLVED, (1.0, 1.0), hyp, None),
              (5, "left"): (OUTSIDE, SOLVED, (-2.0, 0.5), 2.0, 1), (5, "right"): (OUTSIDE, SOLVED, (2.0, 0.5), 2.0, 1),
              (5, "unit"): (INSIDE, SOLVED, (0.0, 0.5), 0.0, 0), (5, "far"): None,
              (6, "diag"): (OUTSIDE, SOLVED, (9.5, 10.5), 3 * s, 1), (6, "far"): None}
    return list(regs), list(regs.values()), pts, rad, expect


def beyond_case():
    """a candidate whose lower bound passes and whose distance does not (status 1): the unit square and a point off its corner on the
    diagonal, every row violated by 0.5 and the corner 0.5 sqrt(2) away, radius 0.6"""
    return [_box((0, 0), (1, 1))], np.array([[1.5, 1.5]]), np.array([0.6]), float(0.5 * np.sqrt(2.0))


# ------------------------------------------------------------------------------------------- the host build
_emu = []


def emu():
    """tests/hostemu/project_emu.cpp against csrc/point_project_core.h, rebuilt when a source changes.  -ffp-contract=off: only the
    written fma calls fuse, as in the kernels"""
    if not _emu:
        so = build_library(os.path.join(hostemu_lib.HOSTEMU, "libprojectemu.so"), hostemu_lib.sources([("project_emu.cpp", [])]),
                           flags=hostemu_lib.FLAGS + ["-ffp-contract=off"])
        lib = C.CDLL(so)
        lib.project_emu_call.restype = C.c_longlong
        lib.project_emu_call.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_longlong]
        lib.project_emu_pair.restype = C.c_int
        lib.project_emu_pair.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 4
        lib.project_emu_chunk.restype = C.c_int
        _emu.append(lib)
    return _emu[0]


FIELDS = ("hit_ptr", "hit_region", "hit_class", "distance", "nearest", "status", "iterations")


def emu_project(polys, pts, radius=None, max_iter=MAX_ITER, n=None):
    """(hit_ptr, hit_region, hit_class, distance, nearest, status, iterations) of the host build: the contract of ``DeviceScene.project``"""
    lib = emu()
    pts = np.ascontiguousarray(pts, float)
    n = n if n is not None else pts.shape[1]
    pts = pts.reshape(-1, n)
    rad = None if radius is None else np.ascontiguousarray(radius, float)
    ptr, A, b = lc.csr(polys, n)
    num, P = len(pts), len(polys)
    hit_ptr = np.zeros(num + 1, np.int64)
    args = (n, P, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, num, pts.ctypes.data, None if rad is None else rad.ctypes.data, int(max_iter), hit_ptr.ctypes.data)
    T = lib.project_emu_call(*args, None, None, None, None, None, None, -1)
    assert T >= 0, T
    out = (np.empty(T, np.int32), np.empty(T, np.uint8), np.empty(T), np.empty((T, n)), np.empty(T, np.int32), np.empty(T, np.int32))
    assert lib.project_emu_call(*args, *(a.ctypes.data for a in out), T) == T
    return (hit_ptr,) + out


def double_loop(polys, pts, radius, max_iter=MAX_ITER):
    """the seven arrays a plain loop over points, then regions makes of the classification and the solve of every pair"""
    lib = emu()
    n = pts.shape[1]
    ptr, A, b = lc.csr(polys, n)
    pts = np.ascontiguousarray(pts, float)
    hit_ptr, region, cls, dist, near, status, its = [0], [], [], [], [], [], []
    x = np.zeros(n); d = C.c_double(0); st = C.c_int(0); it = C.c_int(0)
    for q in range(len(pts)):
        for r in range(len(polys)):
            k = lib.project_emu_pair(n, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, r, pts[q].ctypes.data, float(radius[q]), int(max_iter), x.ctypes.data,
                                     C.addressof(d), C.addressof(st), C.addressof(it))
            assert k in (OUT, INSIDE, OUTSIDE)
            if k != OUT:
                region.append(r); cls.append(k); dist.append(d.value); near.append(x.copy()); status.append(st.value); its.append(it.value)
        hit_ptr.append(len(region))
    return (np.array(hit_ptr, np.int64), np.array(region, np.int32), np.array(cls, np.uint8), np.array(dist, float),
            np.array(near, float).reshape(-1, n), np.array(status, np.int32), np.array(its, np.int32))


def dense(res, num, P):
    """(class [Q, P] with 0 for a pair that is not listed, list position [Q, P] or -1) after the list's own checks (locate_cases.dense)"""
    M = lc.dense(res[:3], num, P)
    at = np.full((num, P), -1, np.int64)
    point_of = np.repeat(np.arange(num, dtype=np.int64), np.diff(res[0]))
    at[point_of, res[1]] = np.arange(len(res[1]))
    return M, at


_cache = {}


def family(kind, n, P, offset, num=Q):
    """(polys, points, radii, the host build's seven arrays) of one family member, the arrays computed once and left unchanged (the
    device tests compare with them)"""
    key = (kind, n, P, offset, num)
    if key not in _cache:
        polys, pts, rad = lc.regions(kind, n, P, offset), lc.points(kind, n, P, offset, Q)[:num], radii(Q)[:num]
        res = emu_project(polys, pts, rad)
        for a in res:
            a.setflags(write=False)
        _cache[key] = (polys, pts, rad, res)
    return _cache[key]
