"""Boxes, crafted cases and the host build for the tests of locate_box_kernel (csrc/box_locate_core.h), shared by the host-build tests
(test_locate_boxes.py) and the device tests (test_gpu_locate_boxes.py).  The regions are those of locate_cases.py, imported.

``boxes(kind, n, P, offset, Q)``: centres as ``locate_cases.points`` draws its points (even: uniform over the domain, odd: around a
region), half-widths log-uniform per axis from 5e-5 (a box 1e-4 wide) to 2 (several regions wide: the regions' half-widths are 0.05 ..
0.9).  The seeds are fixed."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import hostemu_lib
import locate_cases as lc
from gcs_admm_amd.native_build import build_library

OUT, IN, UNDECIDED = lc.OUT, lc.IN, lc.UNDECIDED
TOL = lc.TOL


def boxes(kind, n, P, offset=0.0, Q=12):
    """(lo [Q, n], hi [Q, n])"""
    c = lc.points(kind, n, P, offset, Q)
    rng = np.random.default_rng(lc._seed(kind, n, P, offset) + 13)
    h = 10.0 ** rng.uniform(np.log10(5e-5), np.log10(2.0), (Q, n))
    h[0], h[1 % Q] = 5e-5, 2.0          # both ends of the range are always there (box 1 is one around a region)
    return np.ascontiguousarray(c - h), np.ascontiguousarray(c + h)


def region_box(A, b, n):
    """(lo, hi) of the box rows every region of locate_cases starts with (rows 0 .. 2n: +e_k then -e_k, possibly scaled)"""
    k = np.arange(n)
    return b[n + k] / A[n + k, k], b[k] / A[k, k]


def interior_boxes(polys, n):
    """one box per region, wholly inside it: centred at the centre c of the region's box rows, half-width 0.4 rad / sqrt(n) where rad
    = min_i (b_i - a_i.c) / |a_i|_2 is the radius of the largest ball about c in the region, so that every point of the box is at least
    rad - 0.4 rad = 0.6 rad >= rad / 2 from every facet.  (lo [P, n], hi [P, n], rad [P])"""
    lo, hi, rad = [], [], []
    for A, b in polys:
        rl, rh = region_box(A, b, n)
        c = 0.5 * (rl + rh)
        r = float(np.min((b - A @ c) / np.linalg.norm(A, axis=1)))
        assert r > 0
        t = 0.4 * r / np.sqrt(n)
        lo.append(c - t); hi.append(c + t); rad.append(r)
    return np.array(lo), np.array(hi), np.array(rad)


def _box(lo, hi):
    return np.vstack([np.eye(2), -np.eye(2)]), np.array([hi[0], hi[1], -lo[0], -lo[1]], float)


def crafted():
    """(names, polys, lo, hi, expect, overlap): n = 2.  ``expect[(box, region name)]`` is the class the classifier must report and
    ``overlap[(box, region name)]`` whether box and region share a point."""
    regs = {"unit": _box((0, 0), (1, 1)), "wedge": lc.WEDGE, "small": _box((0.1, 0.1), (0.3, 0.3)), "far": _box((50, 50), (51, 51)),
            "around": _box((-1e3, -1e3), (1e3, 1e3))}
    bx = [((1.0, 0.2), (2.0, 0.8)),                   # 0 touches the facet x = 1 of unit
          ((1.0, 1.0), (2.0, 2.0)),                   # 1 touches the vertex (1, 1) of unit
          ((1.0 + 1e-6, 0.2), (2.0, 0.8)),            # 2 a gap of 1e-6 to that facet
          ((0.0, 0.0), (4.0, 4.0)),                   # 3 contains `small` whole; its centre (2, 2) misses it
          ((0.4, 0.4), (0.6, 0.6)),                   # 4 deep inside unit
          ((-2.0, -1.0), (-1e-5, 1.0)),               # 5 just beyond the wedge's acute vertex: every row alone admits a point of it
          ((0.2 - 5e-5, 0.2 - 5e-5), (0.2 + 5e-5, 0.2 + 5e-5)),      # 6 1e-4 wide, inside small
          ((-5.0, -5.0), (60.0, 60.0))]               # 7 several regions wide: meets everything
    lo = np.array([b[0] for b in bx], float); hi = np.array([b[1] for b in bx], float)
    expect = {(0, "unit"): UNDECIDED, (1, "unit"): UNDECIDED, (2, "unit"): OUT, (3, "small"): UNDECIDED, (3, "unit"): UNDECIDED,
              (4, "unit"): IN, (4, "small"): OUT, (5, "wedge"): UNDECIDED, (6, "small"): IN, (6, "unit"): IN, (7, "small"): UNDECIDED,
              (7, "far"): UNDECIDED, (3, "far"): OUT}
    expect.update({(q, "around"): IN for q in range(len(bx))})
    overlap = {(0, "unit"): True, (1, "unit"): True, (2, "unit"): False, (3, "small"): True, (3, "unit"): True, (4, "unit"): True,
               (4, "small"): False, (5, "wedge"): False, (6, "small"): True, (7, "far"): True, (3, "far"): False}
    return list(regs), list(regs.values()), lo, hi, expect, overlap


def box_polytope(lo, hi):
    """the box as the polytope [I; -I] x <= [hi; -lo]"""
    n = len(lo)
    return np.vstack([np.eye(n), -np.eye(n)]), np.hstack([hi, -np.asarray(lo)])


# ------------------------------------------------------------------------------------------- the host build
_emu = []


def emu():
    """tests/hostemu/locate_box_emu.cpp against csrc/box_locate_core.h, rebuilt when a source changes.  -ffp-contract=off: only the
    written fma calls fuse, as in the kernel"""
    if not _emu:
        so = build_library(os.path.join(hostemu_lib.HOSTEMU, "liblocateboxemu.so"), hostemu_lib.sources([("locate_box_emu.cpp", [])]),
                           flags=hostemu_lib.FLAGS + ["-ffp-contract=off"])
        lib = C.CDLL(so)
        lib.locate_box_emu_hits.restype = C.c_longlong
        lib.locate_box_emu_hits.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
        lib.locate_box_emu_class.restype = C.c_int
        lib.locate_box_emu_class.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double]
        lib.locate_box_emu_chunk.restype = C.c_int
        _emu.append(lib)
    return _emu[0]


def emu_locate_boxes(polys, lo, hi, tol=TOL, n=None):
    """(hit_ptr, hit_region, hit_class) of the host build: the count first, then the list -- the contract of ``DeviceScene.locate_boxes``"""
    lib = emu()
    lo = np.ascontiguousarray(lo, float); hi = np.ascontiguousarray(hi, float)
    n = n if n is not None else lo.shape[1]
    lo = lo.reshape(-1, n); hi = hi.reshape(-1, n)
    ptr, A, b = lc.csr(polys, n)
    Q, P = len(lo), len(polys)
    hit_ptr = np.zeros(Q + 1, np.int64)
    args = (n, P, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, Q, lo.ctypes.data, hi.ctypes.data, tol, hit_ptr.ctypes.data)
    T = lib.locate_box_emu_hits(*args, None, None, -1)
    assert T >= 0, T
    hit_region = np.empty(T, np.int32); hit_class = np.empty(T, np.uint8)
    assert lib.locate_box_emu_hits(*args, hit_region.ctypes.data, hit_class.ctypes.data, T) == T
    return hit_ptr, hit_region, hit_class


def double_loop(polys, lo, hi, tol=TOL):
    """the list a plain loop over boxes, then regions makes of the class of every pair (locate_box_classify called pair by pair)"""
    lib = emu()
    n = lo.shape[1]
    ptr, A, b = lc.csr(polys, n)
    lo = np.ascontiguousarray(lo, float); hi = np.ascontiguousarray(hi, float)
    hit_ptr, region, cls = [0], [], []
    for q in range(len(lo)):
        for r in range(len(polys)):
            k = lib.locate_box_emu_class(n, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, r, lo[q].ctypes.data, hi[q].ctypes.data, tol)
            assert k in (OUT, IN, UNDECIDED)
            if k != OUT:
                region.append(r); cls.append(k)
        hit_ptr.append(len(region))
    return np.array(hit_ptr, np.int64), np.array(region, np.int32), np.array(cls, np.uint8)


_cache = {}


def family_hits(kind, n, P, offset, Q, of=12):
    """the host build's list for the first Q of the ``of`` boxes of one family member, computed once (the device tests compare with it)"""
    key = (kind, n, P, offset, Q, of)
    if key not in _cache:
        lo, hi = boxes(kind, n, P, offset, of)
        _cache[key] = emu_locate_boxes(lc.regions(kind, n, P, offset), lo[:Q], hi[:Q])
    return _cache[key]
