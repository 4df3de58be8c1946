"""Pair lists, hit lists, the host build and the references for the tests of the device assembly of query graphs
(csrc/query_graph_core.h; gcsadmm_scene_build_region_graph / _read_region_graph / _query_graphs in csrc/polytope_lp.hip), shared by
test_query_graph.py (host build, no GPU) and test_gpu_query_graph.py.

References: the region graph is ``gcs_admm_amd.scene.edge_arrays`` element for element, with rows and reverse edges that must agree
with it; a query graph is ``host_query_graph``: the lines of ``SceneQueries.graphs`` that merge the terminal edges into the region
edges, then ``graph._finish_graph`` itself (it is the definition), all seven arrays by dtype and bytes."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import sweep_cases as S
from gcs_admm_amd.graph import _finish_graph
from hostemu_lib import emu_library
from gcs_admm_amd.scene import candidate_pairs, edge_arrays, query_graph_views

ROOT = S.ROOT
EMU_SRC = os.path.join(ROOT, "tests", "hostemu", "query_graph_emu.cpp")
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2

REGIONS = (1, 2, 63, 64, 65, 130, 600)
BATCHES = (1, 2, 5, 130)
DENSITIES = (0.0, 0.1, 1.0)
CHUNKS = (0, 1, 3)
ARRAYS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head")


# ------------------------------------------------------------------------------------------- pair lists
def box_polys(lo, hi):
    n = lo.shape[1]
    A = np.vstack([np.eye(n), -np.eye(n)])
    return [(A, np.hstack([h, -l])) for l, h in zip(lo, hi)]


def scene_boxes(name):
    """(lo, hi) of a named scene of boxes: ``boxes<P>`` (sweep_cases.boxes at n = 2), ``identical`` (330 equal boxes: every pair),
    ``hub`` (box 0 around 599 disjoint others: one row of degree 599), ``apart`` (130 disjoint boxes: no pair at all)"""
    if name.startswith("boxes"):
        return S.boxes(2, int(name[5:]))
    if name == "identical":
        return np.zeros((330, 3)), np.ones((330, 3))
    if name == "hub":
        lo = np.zeros((600, 2)); lo[1:, 0] = 2.0 * np.arange(1, 600); lo[1:, 1] = 1.0
        hi = lo + 1.0
        lo[0], hi[0] = (-5.0, -5.0), (1300.0, 5.0)
        return lo, hi
    assert name == "apart", name
    lo = np.arange(130, dtype=float)[:, None] * np.array([[2.0, 0.0]])
    return lo, lo + 1.0


def scene_pairs(name, shuffled=False):
    """(P, pa, pb) of the boxes' candidate pairs at pad 0 (for boxes: exactly the pairs that overlap), in sweep order or shuffled"""
    lo, hi = scene_boxes(name)
    pa, pb = candidate_pairs(lo, hi, 0.0)
    if shuffled:
        o = np.random.default_rng(len(pa) + 3).permutation(len(pa))
        pa, pb = pa[o], pb[o]
    return lo.shape[0], np.ascontiguousarray(pa, np.int32), np.ascontiguousarray(pb, np.int32)


def random_flags(T, density, seed=0):
    """uint8 [T]: 0 or a non-zero value (1 or 255: any non-zero flag is an overlap)"""
    rng = np.random.default_rng(1000 + T + seed)
    on = rng.random(T) < density
    return np.where(on, np.where(rng.random(T) < 0.5, 1, 255), 0).astype(np.uint8)


SCENES = ["boxes%d" % P for P in REGIONS] + ["identical", "hub", "apart"]


# ------------------------------------------------------------------------------------------- hit lists
def hit_lists(P, B, degree, seed=0):
    """(term_ptr int64 [2B + 1], term_region int32, st uint8 [B]) of B queries on P regions: lists of 1, 2 and 10 regions (fewer where P
    has fewer), strictly ascending.  Query 0: the goal's list shares its regions with the start's; query 1: rs == rt with c = 1 (start =
    goal); query 2: the first and the last region; query 3: a region of degree 0 where there is one.  c is drawn for the others."""
    rng = np.random.default_rng(77 * P + B + seed)
    sizes = (1, 2, 10)
    pick = lambda q: np.sort(rng.choice(P, size=min(P, sizes[(q + seed) % 3]), replace=False))
    lists = [pick(q) for q in range(2 * B)]
    st = (rng.random(B) < 0.4).astype(np.uint8)
    lone = np.nonzero(np.asarray(degree) == 0)[0]
    lists[B] = np.union1d(lists[0], pick(0))
    if B >= 2:
        lists[B + 1] = lists[1].copy(); st[1] = 1
    else:
        st[0] = seed % 2
    if B >= 3:
        lists[2] = np.union1d(lists[2], [0]); lists[B + 2] = np.union1d(lists[B + 2], [P - 1])
    if B >= 4 and len(lone):
        lists[3] = np.union1d(lists[3], lone[:1]); lists[B + 3] = np.array([lone[-1]])
    term_ptr = np.zeros(2 * B + 1, np.int64)
    term_ptr[1:] = np.cumsum([len(l) for l in lists])
    return term_ptr, np.concatenate(lists).astype(np.int32), st


# ------------------------------------------------------------------------------------------- the references
def check_region_graph(got, P, pa, pb, flags):
    """``got`` = (row_ptr, tail, head, rev) against scene.edge_arrays, with rows and reverse edges that agree with it"""
    row_ptr, tail, head, rev = got
    rt, rh = edge_arrays(pa, pb, flags)
    assert row_ptr.dtype == np.int64 and tail.dtype == head.dtype == rev.dtype == np.int32
    assert tail.tobytes() == rt.tobytes() and head.tobytes() == rh.tobytes(), (len(tail), len(rt))
    want = np.zeros(P + 1, np.int64)
    want[1:] = np.cumsum(np.bincount(rt, minlength=P))
    assert np.array_equal(row_ptr, want)
    assert len(rev) == 0 or (rev.min() >= 0 and rev.max() < len(rev))
    assert np.array_equal(tail[rev], head) and np.array_equal(head[rev], tail)


def host_query_graph(edge_tail, edge_head, P, rs, rt, c):
    """the seven arrays of one query graph as the host path makes them: the merge of ``SceneQueries.graphs`` (region edges shifted by
    two, both directions of every hit, both of s-t if the boxes meet, one lexsort), then ``graph._finish_graph``"""
    rs, rt = np.asarray(rs, np.int64) + 2, np.asarray(rt, np.int64) + 2
    st = np.array([0], np.int64) if c else np.zeros(0, np.int64)
    zs, zt = np.zeros(len(rs), np.int64), np.ones(len(rt), np.int64)
    tail = np.concatenate([edge_tail.astype(np.int64) + 2, zs, rs, zt, rt, st, st + 1])
    head = np.concatenate([edge_head.astype(np.int64) + 2, rs, zs, rt, zt, st + 1, st])
    o = np.lexsort((head, tail))
    one = (np.zeros((1, 1)), np.zeros(1))
    g = _finish_graph(1, list(range(P + 2)), tail[o], head[o], [one] * (P + 2), np.zeros((P + 2, 1)), 0, 1)
    return tuple(getattr(g, f) for f in ARRAYS)


def check_query_graphs(got, edge_tail, edge_head, P, term_ptr, term_region, st):
    """every query of ``got`` (tuples of seven arrays) against host_query_graph, dtype and bytes"""
    B = len(st)
    assert len(got) == B
    for i in range(B):
        rs = term_region[term_ptr[i]:term_ptr[i + 1]]; rt = term_region[term_ptr[B + i]:term_ptr[B + i + 1]]
        ref = host_query_graph(edge_tail, edge_head, P, rs, rt, int(st[i]))
        for f, a, b in zip(ARRAYS, got[i], ref):
            assert a.dtype == b.dtype == np.int32 and a.shape == b.shape, (i, f, a.shape, b.shape)
            assert a.tobytes() == b.tobytes(), (i, f, np.nonzero(a != b)[0][:5])


def same_bytes(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for p, q in zip(a, b) for x, y in zip(p, q))


# ------------------------------------------------------------------------------------------- the host build
_p, _i, _ll = C.c_void_p, C.c_int, C.c_longlong
QUERY_ARGS = [_p, _i, _p, _p, _p, _i, _p] + [_p] * 7


def declare(lib):
    lib.qg_emu_create.restype = _p
    lib.qg_emu_create.argtypes = [_i, _ll, _p, _p, _p]
    lib.qg_emu_destroy.restype = None
    lib.qg_emu_destroy.argtypes = [_p]
    lib.qg_emu_last_error.restype = C.c_char_p
    lib.qg_emu_last_error.argtypes = [_p]
    lib.qg_emu_invalidate.restype = None
    lib.qg_emu_invalidate.argtypes = [_p]
    lib.qg_emu_build.restype = _i
    lib.qg_emu_build.argtypes = [_p, _p, _p]
    lib.qg_emu_read.restype = _i
    lib.qg_emu_read.argtypes = [_p] * 5
    lib.qg_emu_query.restype = _i
    lib.qg_emu_query.argtypes = QUERY_ARGS
    lib.qg_emu_scan.restype = _i
    lib.qg_emu_scan.argtypes = [_p, _i, _p]
    lib.qg_emu_chunk.restype = _i
    lib.qg_emu_chunk.argtypes = [_i, _ll, _i]
    return lib


def load_query_graph_emu():
    """tests/hostemu/query_graph_emu.cpp against csrc/query_graph_core.h, rebuilt when a source changes"""
    return declare(emu_library("querygraphemu"))


_emu = []


def emu():
    if not _emu:
        _emu.append(load_query_graph_emu())
    return _emu[0]


class EmuError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"{text} (status {status})")
        self.status = status


class EmuGraph:
    """the three calls on a pair list handed in, through the host build: ``build_region_graph``, ``region_graph`` and ``query_graphs``
    with the signatures of ``scene.DeviceScene``; a status other than 0 raises EmuError"""

    def __init__(self, P, pa, pb, flags, lib=None):
        self.lib = lib or emu()
        self.P = P
        self.pa, self.pb = np.ascontiguousarray(pa, np.int32), np.ascontiguousarray(pb, np.int32)
        self.flags = np.ascontiguousarray(flags, np.uint8)
        self.h = self.lib.qg_emu_create(P, len(self.pa), self.pa.ctypes.data, self.pb.ctypes.data, self.flags.ctypes.data)
        self.num_region_edges = 0

    def close(self):
        if self.h:
            self.lib.qg_emu_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def check(self, rc):
        if rc:
            raise EmuError(rc, self.lib.qg_emu_last_error(self.h).decode())

    def invalidate(self):
        self.lib.qg_emu_invalidate(self.h)

    def build_region_graph(self, flags=None):
        f = None if flags is None else np.ascontiguousarray(flags, np.uint8)
        num = C.c_longlong(-1)
        self.check(self.lib.qg_emu_build(self.h, f.ctypes.data if f is not None else None, C.addressof(num)))
        self.num_region_edges = int(num.value)
        return self.num_region_edges

    def region_graph(self):
        row_ptr = np.empty(self.P + 1, np.int64)
        self.check(self.lib.qg_emu_read(self.h, row_ptr.ctypes.data, None, None, None))
        E = int(row_ptr[-1])
        tail = np.empty(E, np.int32); head = np.empty(E, np.int32); rev = np.empty(E, np.int32)
        self.check(self.lib.qg_emu_read(self.h, None, tail.ctypes.data, head.ctypes.data, rev.ctypes.data))
        return row_ptr, tail, head, rev

    def query_graphs(self, term_ptr, term_region, st_adjacent, chunk_queries=0):
        return query_graph_views(self.P, self.num_region_edges, term_ptr, term_region, st_adjacent,
                                 lambda *a: self.check(self.lib.qg_emu_query(self.h, *a)), chunk_queries)


def raw_outputs(B, P, E_total, fill=-3):
    """the seven flat output arrays of a call, filled with a value no entry takes"""
    sizes = (E_total, E_total, B * (P + 3), 2 * E_total, 2 * E_total, E_total, E_total)
    return [np.full(max(s, 1), fill, np.int32) for s in sizes]


def edge_offsets(E_R, term_ptr, st):
    B = len(st)
    hits = np.diff(term_ptr)
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(E_R + 2 * (hits[:B] + hits[B:]) + 2 * (np.asarray(st) != 0))
    return off


def refusals(P, E_R, term_ptr, term_region, st):
    """(label, status, text, arguments num_queries .. edge_off of a query_graphs call) for every refusal the header lists, made from a
    valid call on a region graph with E_R edges; needs B >= 2 and a first list of two regions or more"""
    B = len(st)
    off = edge_offsets(E_R, term_ptr, st)
    assert B >= 2 and term_ptr[1] >= 2
    ok = dict(B=B, ptr=term_ptr, reg=term_region, st=st, chunk=0, off=off)
    def case(label, status, text, **change):
        a = dict(ok, **{k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in change.items()})
        return label, status, text, a
    down = term_ptr.copy(); down[1] = term_ptr[2] + 1                      # term_ptr[2] < term_ptr[1]
    shifted = term_ptr + 1
    twice = term_region.copy(); twice[1] = twice[0]                         # the first list is not STRICTLY ascending
    swapped = term_region.copy(); swapped[[0, 1]] = swapped[[1, 0]]
    high = term_region.copy(); high[term_ptr[1] - 1] = P                    # the largest entry of the first list leaves [0, P)
    low = term_region.copy(); low[0] = -1
    c2 = st.copy(); c2[0] = 2
    short = off.copy(); short[1:] -= 1
    many = term_ptr.copy(); many[-1] = 2 ** 31                             # more hits than an int32 counts (nothing is read from them)
    return [case("negative num_queries", BAD_ARG, "negative", B=-1),
            case("negative chunk", BAD_ARG, "negative", chunk=-1),
            case("term_ptr decreasing", BAD_ARG, "non-decreasing", ptr=down),
            case("term_ptr not from 0", BAD_ARG, r"term_ptr\[0\]", ptr=shifted),
            case("list with a repeat", BAD_ARG, "strictly ascending", reg=twice),
            case("list descending", BAD_ARG, "strictly ascending", reg=swapped),
            case("region = P", BAD_ARG, "out of range", reg=high),
            case("region < 0", BAD_ARG, "out of range", reg=low),
            case("st_adjacent = 2", BAD_ARG, "neither 0 nor 1", st=c2),
            case("edge_off one short", BAD_ARG, "edge_off", off=short),
            case("null term_ptr", BAD_ARG, "null", ptr=None),
            case("2^31 hits", UNSUPPORTED, "hits", ptr=many)]
