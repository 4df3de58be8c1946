"""Boxes, the host build and the checks for the tests of scene edits (csrc/scene_edit_core.h; gcsadmm_scene_add_regions and
gcsadmm_scene_remove_regions in csrc/polytope_lp.hip), shared by test_scene_edit.py (host build, no GPU) and test_gpu_scene_edit.py.
The reference of both is ``gcs_admm_amd.scene.candidate_pairs`` on the edited set of boxes: the contract is its pair list element for
element, with the flag and status of every pair that was there before the edit."""
from __future__ import annotations

import ctypes as C

import numpy as np

import sweep_cases as S
from hostemu_lib import emu_library
from gcs_admm_amd.scene import candidate_pairs


DIMS = (1, 2, 8)
RESIDENT = (0, 1, 63, 64, 65, 200)
APPENDED = (0, 1, 64, 130)
NEW_FLAG, NEW_STATUS = 255, -9          # what the host build marks a new pair with (on the device its LP has run by then)


def random_boxes(n, count):
    return S.boxes(n, count)


def lattice_boxes(n, count, seed=3):
    """unit boxes on the integer lattice (a row at n = 1, a near-square grid in the first two coordinates otherwise) in shuffled order:
    neighbours touch, and whole columns tie in the sort key"""
    w = max(1, int(np.ceil(np.sqrt(count)))) if n > 1 else max(count, 1)
    k = np.arange(count)
    lo = np.zeros((count, n))
    lo[:, 0] = k % w
    if n > 1:
        lo[:, 1] = k // w
    lo = lo[np.random.default_rng(seed + 10 * n + count).permutation(count)]
    return lo, lo + 1.0


def tags(T):
    """a distinct (flag, status) for every resident pair; no flag equals NEW_FLAG"""
    t = np.arange(T)
    return (t % 251).astype(np.uint8), (1000 + t).astype(np.int32)


# ------------------------------------------------------------------------------------------- the host build
def load_edit_emu():
    """tests/hostemu/scene_edit_emu.cpp against csrc/scene_edit_core.h, rebuilt when a source changes"""
    lib = emu_library("sceneeditemu")
    p, i, ll, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    lib.edit_emu_add.restype = ll
    lib.edit_emu_add.argtypes = [i, i, i, p, p, d, ll, p, p, p, p, p, p, p, p, ll, p]
    lib.edit_emu_remove.restype = ll
    lib.edit_emu_remove.argtypes = [i, i, p, p, d, i, p, ll, p, p, p, p, p, p, p, p, p]
    lib.edit_emu_scan.restype = i
    lib.edit_emu_scan.argtypes = [p, ll, p]
    return lib


def _list(pa, pb, flag, st):
    return tuple(np.ascontiguousarray(a, t) for a, t in ((pa, np.int32), (pb, np.int32), (flag, np.uint8), (st, np.int32)))


def emu_add(lib, lo, hi, P, pad, resident):
    """the list (pa, pb, flag, status) after boxes P .. of lo, hi are added to a scene that holds ``resident`` = (pa, pb, flag, status)
    of boxes 0 .. P-1, and the number of new pairs: the length first, then the list"""
    lo = np.ascontiguousarray(lo, float); hi = np.ascontiguousarray(hi, float)
    n, K = lo.shape[1], lo.shape[0] - P
    pa, pb, flag, st = _list(*resident)
    new = C.c_longlong(0)
    head = (n, P, K, lo.ctypes.data, hi.ctypes.data, pad, len(pa), pa.ctypes.data, pb.ctypes.data, flag.ctypes.data, st.ctypes.data)
    T = lib.edit_emu_add(*head, None, None, None, None, -1, C.addressof(new))
    assert T >= 0, T
    out = _list(*(np.zeros(T) for _ in range(4)))
    assert lib.edit_emu_add(*head, *(a.ctypes.data for a in out), T, C.addressof(new)) == T
    return out, int(new.value)


def emu_remove(lib, lo, hi, pad, regions, resident):
    """(newidx, (pa, pb, flag, status)) after ``regions`` are removed; None if the host build refuses the indices"""
    lo = np.ascontiguousarray(lo, float); hi = np.ascontiguousarray(hi, float)
    P, n = lo.shape
    pa, pb, flag, st = _list(*resident)
    regions = np.ascontiguousarray(regions, np.int32)
    newidx = np.empty(P, np.int32)
    out = _list(*(np.zeros(len(pa)) for _ in range(4)))
    T = lib.edit_emu_remove(n, P, lo.ctypes.data, hi.ctypes.data, pad, len(regions), regions.ctypes.data, len(pa), pa.ctypes.data, pb.ctypes.data,
                            flag.ctypes.data, st.ctypes.data, newidx.ctypes.data, *(a.ctypes.data for a in out))
    if T == -1:
        return None
    assert T >= 0, T
    return newidx, tuple(a[:T] for a in out)


# ------------------------------------------------------------------------------------------- the checks
def tagged_pairs(lo, hi, pad):
    pa, pb = candidate_pairs(lo, hi, pad)
    return (pa, pb) + tags(len(pa))


def check_added(got, num_new, lo, hi, P, pad, resident):
    """``got`` is candidate_pairs on all boxes; a pair of two resident boxes carries the tag it had, every other one the new mark"""
    pa, pb, flag, st = got
    ra, rb = candidate_pairs(lo, hi, pad)
    assert pa.dtype == pb.dtype == np.int32
    assert np.array_equal(pa, ra) and np.array_equal(pb, rb), (len(pa), len(ra))
    new = pb >= P
    assert int(new.sum()) == num_new == len(pa) - len(resident[0])
    assert np.all(flag[new] == NEW_FLAG) and np.all(st[new] == NEW_STATUS)
    had = {(a, b): (f, s) for a, b, f, s in zip(*(x.tolist() for x in resident))}
    assert len(had) == len(resident[0])
    assert [had[k] for k in zip(pa[~new].tolist(), pb[~new].tolist())] == list(zip(flag[~new].tolist(), st[~new].tolist()))


def check_removed(newidx, got, lo, hi, pad, regions, resident):
    """``newidx`` renumbers the regions that stay; ``got`` is candidate_pairs on their boxes, every pair with the tag it had"""
    P = lo.shape[0]
    stays = np.ones(P, bool); stays[np.asarray(regions, int)] = False
    want = np.where(stays, np.cumsum(stays) - 1, -1)
    assert np.array_equal(newidx, want)
    pa, pb, flag, st = got
    ra, rb = candidate_pairs(lo[stays], hi[stays], pad)
    assert np.array_equal(pa, ra) and np.array_equal(pb, rb), (len(pa), len(ra))
    back = np.nonzero(stays)[0]
    had = {(a, b): (f, s) for a, b, f, s in zip(*(x.tolist() for x in resident))}
    assert [had[k] for k in zip(back[pa].tolist(), back[pb].tolist())] == list(zip(flag.tolist(), st.tolist()))


def extras_split(pad, which):
    """``sweep_cases.extras(pad)`` reordered so that half of it is resident and half appended: ``which`` = 0 the boxes as they come (65
    resident, 65 appended), 1 in reverse (what was resident is appended).  Ties of the sort key, the -0.0, the opened sides and the
    touching pairs then lie on both sides of the split.  Returns (lo, hi, P)."""
    lo, hi = S.extras(pad)
    if which:
        lo, hi = lo[::-1].copy(), hi[::-1].copy()
    return lo, hi, 65
