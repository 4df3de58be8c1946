"""Boxes for the tests of the device broad phase (csrc/box_sweep_core.h, sweep_kernel in csrc/polytope_lp.hip), shared by the host-build
tests (test_scene_resident.py) and the device tests (test_gpu_scene_resident.py).  The reference of both is
``gcs_admm_amd.scene.candidate_pairs``: the contract is its pair list element for element.

``boxes(n, P)``: centres uniform(0, 8) in the first min(n, 2) coordinates and uniform(-0.2, 0.2) in the rest, half-widths
uniform(0.05, 0.9), seed 10 n + 1.  That makes 4-5 % of all pairs candidates at n = 2, 3, 8 and 21-24 % at n = 1 for P = 65, 130, 1000
(``check_share`` holds every sweep test to 3-30 %, so that neither an empty nor a full answer passes), and at P = 1000 some 700 windows
are longer than one 64-lane stride."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from hostemu_lib import emu_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DIMS = (1, 2, 3, 8)
SIZES = (1, 2, 65, 130, 1000)       # one box, one pair, one wavefront of boxes and one more, two and a tail, windows of several strides


def pads():
    from gcs_admm_amd.scene import SWEEP_PAD
    return (0.0, SWEEP_PAD)


def boxes(n, P):
    rng = np.random.default_rng(10 * n + 1)
    c = rng.uniform(-0.2, 0.2, (P, n))
    c[:, :min(n, 2)] = rng.uniform(0, 8, (P, min(n, 2)))
    w = rng.uniform(0.05, 0.9, (P, n))
    return c - w, c + w


def check_share(P, num_pairs):
    if P >= 65:
        T = P * (P - 1) // 2
        assert 0.03 * T <= num_pairs <= 0.3 * T, (P, num_pairs, T)


# the boxes of extras(): (index, what)
TIES = (5, 17, 29, 41, 53, 66, 78, 90, 101, 113)     # ten boxes with lo[:, 0] = 0; TIES[7] has -0.0, which a radix sort would put first
CONTAINER, LO0_INF, HI0_INF, LO1_INF, HI1_INF = 2, 9, 10, 11, 12
POINTS = (20, 21, 22, 23)
TOUCH0, TOUCH1 = (30, 31), (32, 33)                   # lo_j[d] == hi_i[d] + pad exactly, in d = 0 and in d = 1


def extras(pad):
    """``boxes(2, 130)`` with: ties in the sort key (one of them -0.0 among +0.0); a box open to -inf and one open to +inf in each
    coordinate; a box around all others, first in the sweep order (window = P - 1); four 1e-6 point boxes; in each coordinate a pair
    that touches exactly at the padded bound (kept: the tests are <=)."""
    lo, hi = boxes(2, 130)
    lo[list(TIES), 0] = 0.0
    lo[TIES[7], 0] = -0.0
    lo[CONTAINER] = (-np.inf, -1e3); hi[CONTAINER] = (1e3, 1e3)
    lo[LO0_INF, 0] = -np.inf; hi[HI0_INF, 0] = np.inf
    lo[LO1_INF, 1] = -np.inf; hi[HI1_INF, 1] = np.inf
    for p in POINTS:
        c = 0.5 * (lo[p] + hi[p])
        lo[p], hi[p] = c - 1e-6, c + 1e-6
    i, j = TOUCH0
    lo[i], hi[i] = (3.0, 3.0), (3.5, 4.0)
    lo[j], hi[j] = (hi[i, 0] + pad, 3.2), (hi[i, 0] + pad + 0.5, 3.7)
    i, j = TOUCH1
    lo[i], hi[i] = (6.0, 1.0), (6.5, 1.5)
    lo[j], hi[j] = (6.1, hi[i, 1] + pad), (6.4, hi[i, 1] + pad + 0.5)
    assert np.all(lo <= hi)
    return lo, hi


def check_extras(pa, pb):
    """the touching pairs are in the list, and the box around everything is paired with every other box"""
    got = set(zip(pa.tolist(), pb.tolist()))
    assert TOUCH0 in got and TOUCH1 in got
    assert sum(1 for a, b in got if CONTAINER in (a, b)) == 129


def brute_force(lo, hi, pad):
    P = lo.shape[0]
    return {(i, j) for i in range(P) for j in range(i + 1, P) if np.all(lo[i] <= hi[j] + pad) and np.all(lo[j] <= hi[i] + pad)}


# ------------------------------------------------------------------------------------------- the host build
def load_sweep_emu():
    """tests/hostemu/sweep_emu.cpp against csrc/box_sweep_core.h, rebuilt when a source changes"""
    lib = emu_library("sweepemu")
    lib.sweep_emu_pairs.restype = C.c_longlong
    lib.sweep_emu_pairs.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_longlong]
    lib.sweep_emu_scan.restype = C.c_int
    lib.sweep_emu_scan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def emu_pairs(lib, lo, hi, pad):
    """(pair_a, pair_b) of the host build: the count first, then the list"""
    lo = np.ascontiguousarray(lo, float); hi = np.ascontiguousarray(hi, float)
    P, n = lo.shape
    T = lib.sweep_emu_pairs(n, P, lo.ctypes.data, hi.ctypes.data, pad, None, None, -1)
    assert T >= 0, T
    pa = np.empty(T, np.int32); pb = np.empty(T, np.int32)
    assert lib.sweep_emu_pairs(n, P, lo.ctypes.data, hi.ctypes.data, pad, pa.ctypes.data, pb.ctypes.data, T) == T
    return pa, pb
