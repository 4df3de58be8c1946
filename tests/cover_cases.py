"""Segments, lattice scenes, crafted cases, the exact reference and the host build for the tests of the segment kernels
(csrc/segment_clip_core.h), shared by the host-build tests (test_segment_clip.py) and the device tests (test_gpu_segment_clip.py).  The
regions and points of the families are those of locate_cases.py, imported.

The reference of a pair is NOT the code under test: ``exact_span`` intersects, in ``fractions.Fraction``, the half-lines
G_i + t H_i <= E_i of the rows with [0, 1], for the two relaxations E_i of the contract -- ``inner``: tol S_i, ``outer``:
tol S_i (1 + 2^-40) + 2^-39 MAG_i, with S_i = sum_k |a_ik| and MAG_i = |b_i| + sum_k |a_ik| (|p_k| + |d_k|) exact -- on the segment
p + t d with d = q - p as a double (the rule rounds it once; from then on it is data).  To keep the rational work to the rows that
matter, a float64 pass first sets aside, with a margin of 2^-20 MAG_i against its own error of at most 2^-48 MAG_i, the rows that
hold along the whole segment under no relaxation at all (they cut neither span) and the pairs with a row that fails along the whole
segment under twice the outer relaxation (both spans empty); G + t H is affine, so its two ends decide both."""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction as F

import numpy as np

import hostemu_lib
import locate_cases as lc
from gcs_admm_amd.native_build import build_library

OUT, WHOLE, PART = 0, 1, 2
COVERED, GAP = 0, 1
TOL = 1e-9
SIZES = (1, 65, 600)          # project_cases.SIZES: one region; a stride and one; three chunks of LOCATE_CHUNK = 256 with a partial last one
Q = 12
FIELDS = ("hit_ptr", "hit_region", "hit_class", "t_in", "t_out", "status", "reach", "chain_ptr", "chain_hit")
ALLOW, ALLOW2 = F(1, 2 ** 40), F(1, 2 ** 39)


def segments(kind, n, P, offset, num=Q):
    """(start, end) [num, n]: the segments between consecutive points of ``locate_cases.points``"""
    pts = lc.points(kind, n, P, offset)[:num + 1]
    return np.ascontiguousarray(pts[:-1]), np.ascontiguousarray(pts[1:])


# ------------------------------------------------------------------------------------------- the exact reference
def _cut(rows, relax):
    """[0, 1] cut by the rows (G, H, relaxation): (lo, hi) in Fraction, or None when nothing is left"""
    lo, hi = F(0), F(1)
    for (G, H), E in zip(rows, relax):
        if H > 0:
            hi = min(hi, (E - G) / H)
        elif H < 0:
            lo = max(lo, (E - G) / H)
        elif G > E:
            return None
        if lo > hi:
            return None
    return lo, hi


def exact_span(A, b, p, d, tol=TOL):
    """(inner, outer): the exact spans of the segment p + t d in the region under the two relaxations of the contract, each (lo, hi)
    in Fraction or None"""
    A, b, p, d = np.asarray(A, float), np.asarray(b, float), np.asarray(p, float), np.asarray(d, float)
    g0 = A @ p - b
    g1 = g0 + A @ d
    S = np.abs(A).sum(axis=1)
    MAG = np.abs(b) + np.abs(A) @ (np.abs(p) + np.abs(d))
    margin = 2.0 ** -20 * MAG
    if np.any(np.minimum(g0, g1) > 2 * (tol * S * (1 + 2.0 ** -40) + 2.0 ** -39 * MAG) + margin):
        return None, None
    near = np.nonzero(~(np.maximum(g0, g1) < -margin))[0]
    pf, df, t = [F(x) for x in p], [F(x) for x in d], F(tol)
    rows, inner, outer = [], [], []
    for i in near:
        a = [F(x) for x in A[i]]
        rows.append((sum(x * y for x, y in zip(a, pf)) - F(b[i]), sum(x * y for x, y in zip(a, df))))
        s = sum(abs(x) for x in a)
        mag = abs(F(b[i])) + sum(abs(x) * (abs(y) + abs(z)) for x, y, z in zip(a, pf, df))
        inner.append(t * s)
        outer.append(t * s * (1 + ALLOW) + ALLOW2 * mag)
    return _cut(rows, inner), _cut(rows, outer)


def exact_spans(polys, start, end, tol=TOL):
    """{(segment, region): (inner, outer)} of every pair whose outer span is not empty"""
    d = end - start
    out = {}
    for q in range(len(start)):
        for r, (A, b) in enumerate(polys):
            inner, outer = exact_span(A, b, start[q], d[q], tol)
            assert outer is not None or inner is None
            if outer is not None:
                out[(q, r)] = (inner, outer)
    return out


def sweep(spans):
    """the greedy sweep of the contract over one segment's spans [(t_in, t_out)] in list order, in whatever arithmetic they are given
    in: (status, reach, chain as indices into ``spans``)"""
    cur, chain = 0, []
    while cur < 1:
        best = None
        for j, (lo, hi) in enumerate(spans):
            if lo <= cur < hi and (best is None or hi > spans[best][1]):
                best = j
        if best is None:
            return GAP, cur, chain
        chain.append(best)
        cur = spans[best][1]
    return COVERED, cur, chain


# ------------------------------------------------------------------------------------------- lattices with a hole
def lattice(n, offset=0.0, rotate=None):
    """boxes [i, i + 1.05] per axis on a 4 x 4 (n = 2) or 3 x 3 x 3 (n = 3) lattice, moved by ``offset``, one cell left out, and 40
    segments with both ends uniform over the lattice's extent.  ``rotate``: an orthogonal R; the regions become {A R' y <= b} and the
    segments y = R x: the same scene in another frame, with no zero among its coefficients"""
    cells = 4 if n == 2 else 3
    hole = (1, 2) if n == 2 else (1, 1, 1)
    I = np.vstack([np.eye(n), -np.eye(n)])
    polys = []
    for idx in np.ndindex(*([cells] * n)):
        if idx == hole:
            continue
        lo = np.array(idx, float) + offset
        polys.append((I, np.hstack([lo + 1.05, -lo])))
    rng = np.random.default_rng(1000 * n + (1 if offset else 0))
    start, end = rng.uniform(0, cells + 0.05, (40, n)) + offset, rng.uniform(0, cells + 0.05, (40, n)) + offset
    if rotate is not None:
        polys = [(np.ascontiguousarray(A @ rotate.T), b) for A, b in polys]
        start, end = start @ rotate.T, end @ rotate.T
    return polys, np.ascontiguousarray(start), np.ascontiguousarray(end)


LATTICES = [(2, 0.0), (2, 300.0), (3, 0.0), (3, 300.0)]


# ------------------------------------------------------------------------------------------- crafted cases (n = 2)
def _box(lo, hi):
    return np.vstack([np.eye(2), -np.eye(2)]), np.array([hi[0], hi[1], -lo[0], -lo[1]], float)


def crafted():
    """(names, polys, start, end, expect): n = 2, tol = 1e-9.  ``expect[q]`` = (status, reach, chain as region names)"""
    regs = {"a": _box((0, 0), (1, 1)), "abut": _box((1, 0), (2, 1)),                      # a and abut only share the face x = 1
            "apart": _box((2 + 1e-6, 0), (3, 1)),                                        # 1e-6 beyond abut
            "tie1": _box((10, 0), (11, 1)), "tie2": _box((10, 0), (11, 1)), "tie3": _box((10.5, 0), (12, 1)),
            "up": _box((20, 0), (21, 1)), "down": _box((20, -1), (21, 0))}               # up and down share the face y = 0
    start = np.array([[0.25, 0.5], [1.25, 0.5], [20.0, 0.0], [0.5, 0.5], [5.0, 5.0], [5.0, 0.5], [10.25, 0.5], [0.5, 0.5]])
    end = np.array([[1.75, 0.5], [2.75, 0.5], [21.0, 0.0], [0.5, 0.5], [5.0, 5.0], [0.5, 0.5], [11.75, 0.5], [5.0, 0.5]])
    # 0: across the face a and abut share: covered through the tol inflation, the chain a, abut
    # 1: from abut to apart: a gap where abut ends, x = 2 + 1e-9 up to the allowance: t = (0.75 + 1e-9) / 1.5
    # 2: along the face up and down share: WHOLE in both, the chain is the first of the two
    # 3: from == to inside a: WHOLE; 4: from == to outside every region: a gap at 0
    # 5: the start lies outside every region: a gap at reach == 0 although the segment ends in a
    # 6: tie1 and tie2 are the same box: the tie in t_out takes the smaller index, then tie3
    # 7: starts in a, leaves the cover where abut ends, 1e-6 before apart: t = (1.5 + 1e-9) / 4.5
    expect = {0: (COVERED, 1.0, ["a", "abut"]), 1: (GAP, (0.75 + 1e-9) / 1.5, ["abut"]), 2: (COVERED, 1.0, ["up"]),
              3: (COVERED, 1.0, ["a"]), 4: (GAP, 0.0, []), 5: (GAP, 0.0, []), 6: (COVERED, 1.0, ["tie1", "tie3"]),
              7: (GAP, (1.5 + 1e-9) / 4.5, ["a", "abut"])}
    return list(regs), list(regs.values()), start, end, expect


def zero_row_case():
    """(names, polys, start, end): the unit square, a region whose only row is 0 x <= 0.5, one with the rows 0 x <= -1 and 0 x <= 1, and
    one without any row; a segment inside the square and one far from it.  The host build takes them; gcsadmm_scene_create refuses
    a zero facet normal and a polytope without rows"""
    zeros = np.zeros((1, 2))
    regs = {"unit": _box((0, 0), (1, 1)), "zero_whole": (zeros, np.array([0.5])), "zero_never": (np.vstack([zeros, zeros]), np.array([-1.0, 1.0])),
            "empty": (np.zeros((0, 2)), np.zeros(0))}
    return list(regs), list(regs.values()), np.array([[0.25, 0.5], [7.0, 7.0]]), np.array([[0.75, 0.5], [9.0, 8.0]])


def collinear(count=130):
    """``count`` boxes [j, j + 1.5] x [0, 1] and the segment along them: every region meets it (more than one stride of hits in the
    chain kernel) and each of them is in the chain"""
    polys = [_box((j, 0), (j + 1.5, 1)) for j in range(count)]
    return polys, np.array([[0.25, 0.5]]), np.array([[count + 0.25, 0.5]])


# ------------------------------------------------------------------------------------------- the host build
_emu = []


def bind(lib):
    lib.clip_emu_call.restype = C.c_longlong
    lib.clip_emu_call.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 9 + [C.c_longlong]
    lib.clip_emu_pair.restype = C.c_int
    lib.clip_emu_pair.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lib.clip_emu_chunk.restype = C.c_int
    return lib


def emu():
    """tests/hostemu/clip_emu.cpp against csrc/segment_clip_core.h, rebuilt when a source changes.  -ffp-contract=off: only the
    written fma calls fuse, as in the kernels"""
    if not _emu:
        so = build_library(os.path.join(hostemu_lib.HOSTEMU, "libclipemu.so"), hostemu_lib.sources([("clip_emu.cpp", [])]),
                           flags=hostemu_lib.FLAGS + ["-ffp-contract=off"])
        _emu.append(bind(C.CDLL(so)))
    return _emu[0]


def emu_clip(polys, start, end, tol=TOL, n=None, lib=None):
    """the nine arrays of the host build: the contract of ``DeviceScene.clip_segments``"""
    lib = lib or emu()
    start, end = np.ascontiguousarray(start, float), np.ascontiguousarray(end, float)
    n = n if n is not None else start.shape[1]
    start, end = start.reshape(-1, n), end.reshape(-1, n)
    ptr, A, b = lc.csr(polys, n)
    num, P = len(start), len(polys)
    hit_ptr = np.zeros(num + 1, np.int64)
    args = (n, P, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, num, start.ctypes.data, end.ctypes.data, float(tol), hit_ptr.ctypes.data)
    T = lib.clip_emu_call(*args, None, None, None, None, None, None, None, None, -1)
    assert T >= 0, T
    region, cls, t_in, t_out = np.empty(T, np.int32), np.empty(T, np.uint8), np.empty(T), np.empty(T)
    status, reach, chain_ptr, chain = np.empty(num, np.int32), np.empty(num), np.zeros(num + 1, np.int64), np.empty(T, np.int32)
    assert lib.clip_emu_call(*args, *(a.ctypes.data for a in (region, cls, t_in, t_out, status, reach, chain_ptr, chain)), T) == T
    return hit_ptr, region, cls, t_in, t_out, status, reach, chain_ptr, chain[:chain_ptr[-1]].copy()


def double_loop(polys, start, end, tol=TOL, lib=None):
    """(hit_ptr, hit_region, hit_class, t_in, t_out) as a plain loop over segments, then regions makes them of single pairs"""
    lib = lib or emu()
    n = start.shape[1]
    ptr, A, b = lc.csr(polys, n)
    start, end = np.ascontiguousarray(start, float), np.ascontiguousarray(end, float)
    hit_ptr, region, cls, t_in, t_out = [0], [], [], [], []
    lo, hi = C.c_double(0), C.c_double(0)
    for q in range(len(start)):
        for r in range(len(polys)):
            k = lib.clip_emu_pair(n, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, r, start[q].ctypes.data, end[q].ctypes.data, float(tol),
                                  C.addressof(lo), C.addressof(hi))
            assert k in (OUT, WHOLE, PART)
            if k != OUT:
                region.append(r); cls.append(k); t_in.append(lo.value); t_out.append(hi.value)
        hit_ptr.append(len(region))
    return np.array(hit_ptr, np.int64), np.array(region, np.int32), np.array(cls, np.uint8), np.array(t_in, float), np.array(t_out, float)


def own_sweep(res):
    """(status, reach, chain_ptr, chain_hit) the Python sweep makes of a call's own spans"""
    hit_ptr, _, _, t_in, t_out = res[:5]
    status, reach, chain_ptr, chain = [], [], [0], []
    for q in range(len(hit_ptr) - 1):
        lo = int(hit_ptr[q])
        st, r, ch = sweep(list(zip(t_in[lo:hit_ptr[q + 1]].tolist(), t_out[lo:hit_ptr[q + 1]].tolist())))
        status.append(st); reach.append(float(r)); chain += [lo + j for j in ch]; chain_ptr.append(len(chain))
    return np.array(status, np.int32), np.array(reach, float), np.array(chain_ptr, np.int64), np.array(chain, np.int32)


_cache = {}


def _frozen(res):
    for a in res:
        a.setflags(write=False)
    return res


def family(kind, n, P, offset, num=Q):
    """(polys, start, end, the host build's nine arrays) of one family member, the arrays computed once and left unchanged (the
    device tests compare with them)"""
    key = (kind, n, P, offset, num)
    if key not in _cache:
        polys = lc.regions(kind, n, P, offset)
        start, end = segments(kind, n, P, offset, Q)
        start, end = start[:num], end[:num]
        _cache[key] = (polys, start, end, _frozen(emu_clip(polys, start, end)))
    return _cache[key]


def lattice_case(n, offset, rotate=None):
    key = ("lattice", n, offset, rotate)
    if key not in _cache:
        import rotated_cases
        polys, start, end = lattice(n, offset, None if rotate is None else rotated_cases.rotation(n, rotate))
        _cache[key] = (polys, start, end, _frozen(emu_clip(polys, start, end)))
    return _cache[key]
