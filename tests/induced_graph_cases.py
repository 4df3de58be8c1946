"""Region graphs, keep flags, hit lists, the host build and the reference for the tests of the device assembly of pruned query graphs
(csrc/induced_graph_core.h; gcsadmm_scene_induced_sizes / _induced_query_graphs in csrc/polytope_lp.hip), shared by
test_induced_graph.py (host build, no GPU) and test_gpu_induced_graph.py.

Reference: ``query_graph_cases.host_query_graph`` on the edge list of ``scene.edge_arrays`` masked and renumbered the way
``SceneQueries._host_graph(keep=...)`` does it, all seven arrays by dtype, shape and bytes; no tolerance anywhere."""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import numpy as np

import hostemu_lib
import query_graph_cases as Q
from gcs_admm_amd.native_build import build_library
from gcs_admm_amd.scene import candidate_pairs, edge_arrays, induced_query_graph_views, induced_size_arrays

ROOT = Q.ROOT
EMU_SRC = os.path.join(hostemu_lib.HOSTEMU, "induced_graph_emu.cpp")
OK, BAD_ARG, UNSUPPORTED = Q.OK, Q.BAD_ARG, Q.UNSUPPORTED
LATTICE = "lattice1000"                  # 25 x 40 unit cells: four tiles of flags, so the carry crosses three times
SCENES = Q.SCENES + [LATTICE]
BATCHES = Q.BATCHES
CHUNKS = Q.CHUNKS
ARRAYS = Q.ARRAYS


# ------------------------------------------------------------------------------------------- region graphs
def scene_boxes(name):
    if name == LATTICE:
        i, j = np.meshgrid(np.arange(25.0), np.arange(40.0), indexing="ij")
        lo = np.stack([i.ravel(), j.ravel()], axis=1)
        return lo, lo + 1.0
    return Q.scene_boxes(name)


def scene_pairs(name):
    """(P, pa, pb) of the boxes' candidate pairs at pad 0: exactly the pairs that overlap"""
    lo, hi = scene_boxes(name)
    pa, pb = candidate_pairs(lo, hi, 0.0)
    return lo.shape[0], np.ascontiguousarray(pa, np.int32), np.ascontiguousarray(pb, np.int32)


def reverse_edges(tail, head):
    """for every edge of a list without repeats the position of the opposite one"""
    where = {(int(u), int(w)): p for p, (u, w) in enumerate(zip(tail, head))}
    return np.array([where[(int(w), int(u))] for u, w in zip(tail, head)], np.int32).reshape(-1)


@functools.lru_cache(maxsize=None)
def region_graph(name):
    """(P, row_ptr int64 [P + 1], tail, head, rev int32) of the boxes' overlaps: ``scene.edge_arrays`` of every pair, with rows and
    reverse edges made here"""
    P, pa, pb = scene_pairs(name)
    tail, head = edge_arrays(pa, pb, np.ones(len(pa), np.uint8))
    row_ptr = np.zeros(P + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(tail, minlength=P))
    rev = reverse_edges(tail, head)
    for a in (row_ptr, tail, head, rev):
        a.setflags(write=False)
    return P, row_ptr, tail, head, rev


# ------------------------------------------------------------------------------------------- batches: keep flags with hit lists
def _lists(lists, st):
    B = len(st)
    ptr = np.zeros(2 * B + 1, np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    return ptr, np.concatenate([np.asarray(l, np.int32) for l in lists]).astype(np.int32), np.asarray(st, np.uint8)


def _force_hits(keep, ptr, reg):
    """the hit regions of every query into its flags: 1 for a start's, 255 for a goal's (any non-zero byte keeps)"""
    B = keep.shape[0]
    for i in range(B):
        keep[i, reg[ptr[i]:ptr[i + 1]]] = 1
        keep[i, reg[ptr[B + i]:ptr[B + i + 1]]] = 255
    return keep


def _prefix(name, B, count, seed):
    """exactly the regions 0 .. count-1 kept (all of them where the scene has fewer), hit lists drawn inside them"""
    P, row_ptr = region_graph(name)[:2]
    k = min(count, P)
    ptr, reg, st = Q.hit_lists(k, B, np.diff(row_ptr)[:k], seed=seed)
    keep = np.zeros((B, P), np.uint8)
    keep[:, :k] = 1
    return keep, ptr, reg, st


def batch(name, B, pattern, seed=None):
    """(keep uint8 [B, P], term_ptr, term_region, st) of a named keep pattern on a scene; None where the scene has no such pattern.
    ``seed``: that of ``query_graph_cases.hit_lists`` (default: one per pattern)"""
    P, row_ptr, tail, head, _ = region_graph(name)
    degree = np.diff(row_ptr)
    rng = np.random.default_rng(P * 31 + B * 7 + len(pattern))
    ptr, reg, st = Q.hit_lists(P, B, degree, seed=len(pattern) if seed is None else seed)
    keep = np.zeros((B, P), np.uint8)
    if pattern == "all":
        keep[:] = 1
        keep[:, ::3] = 200
        return keep, ptr, reg, st
    if pattern == "hits":
        return _force_hits(keep, ptr, reg), ptr, reg, st
    if pattern in ("random0.1", "random0.5"):
        keep[rng.random((B, P)) < float(pattern[6:])] = 1
        return _force_hits(keep, ptr, reg), ptr, reg, st
    if pattern.startswith("first"):                  # first64: regions 0 .. 63
        return _prefix(name, B, int(pattern[5:]), seed=len(pattern))
    if pattern == "every64th":
        keep[:, ::64] = 1
        return _force_hits(keep, ptr, reg), ptr, reg, st
    if pattern == "last":
        keep[:, P - 1] = 1
        return _force_hits(keep, ptr, reg), ptr, reg, st
    if pattern == "hub_dropped":                     # (hub: region 0 has every other region as its neighbour)
        if name != "hub":
            return None
        ptr, reg, st = Q.hit_lists(P - 1, B, degree[1:], seed=3)
        reg = reg + 1
        keep[:, 1::2] = 1
        return _force_hits(keep, ptr, reg), ptr, reg.astype(np.int32), st
    if pattern == "hub_and_three_leaves":
        if name != "hub":
            return None
        kept = [0, 5, 77, 599]
        keep[:, kept] = 1
        lists = [[0, 77] if q % 2 else [5] for q in range(B)] + [[0, 5, 77, 599] if q % 3 else [599] for q in range(B)]
        return (keep,) + _lists(lists, [q % 2 for q in range(B)])
    assert pattern == "lone_hit", pattern              # a kept region with every neighbour dropped, under both points of query 0
    r = int(np.argmax(degree))
    if degree[r] == 0:
        return None
    near = head[row_ptr[r]:row_ptr[r + 1]]
    far = np.setdiff1d(np.arange(P), np.append(near, r))
    keep[:, far[::2]] = 1
    keep[:, r] = 7
    other = [int(far[0])] if len(far) else []
    lists = [[r] for _ in range(B)] + [sorted([r] + other) if q % 2 == 0 else (other or [r]) for q in range(B)]
    return (keep,) + _lists(lists, [1 if q == 0 else 0 for q in range(B)])


SMALL = [s for s in SCENES if s.startswith("boxes") and int(s[5:]) <= 130]


def batches_of(name, pattern):
    """B = 1, 2, 5, 130 on the scenes of at most 130 regions; on the large ones 2 and 5, and 130 where the graphs stay small"""
    if name in SMALL:
        return BATCHES
    return (2, 5, 130) if name == LATTICE and pattern in ("hits", "random0.1", "every64th") else (2, 5)


PATTERNS = ("all", "hits", "random0.1", "random0.5", "first64", "first65", "first256", "first257", "every64th", "last", "hub_dropped",
            "hub_and_three_leaves", "lone_hit")


# ------------------------------------------------------------------------------------------- the reference
def reference(name, keep, ptr, reg, st):
    """``reference_on`` the region graph of a named scene"""
    _, _, tail, head, _ = region_graph(name)
    return reference_on(tail, head, keep, ptr, reg, st)


def reference_on(tail, head, keep, ptr, reg, st):
    """one tuple of the seven arrays per query: host_query_graph on the edge list (tail, head) masked and renumbered"""
    B = len(st)
    out = []
    for i in range(B):
        k = keep[i] != 0
        new = np.cumsum(k) - 1
        both = k[tail] & k[head]
        rs, rt = reg[ptr[i]:ptr[i + 1]], reg[ptr[B + i]:ptr[B + i + 1]]
        out.append(Q.host_query_graph(new[tail[both]].astype(np.int32), new[head[both]].astype(np.int32), int(k.sum()), new[rs], new[rt], int(st[i])))
    return out


def reference_sizes(ref):
    return np.array([len(g[2]) - 3 for g in ref], np.int32), np.array([len(g[0]) for g in ref], np.int64)


def assert_same(got, ref, label=""):
    assert len(got) == len(ref), (label, len(got), len(ref))
    for i, (g, h) in enumerate(zip(got, ref)):
        for f, a, b in zip(ARRAYS, g, h):
            assert a.dtype == b.dtype == np.int32 and a.shape == b.shape, (label, i, f, a.shape, b.shape)
            assert a.tobytes() == b.tobytes(), (label, i, f, np.nonzero(a != b)[0][:5])


same_bytes = Q.same_bytes


# ------------------------------------------------------------------------------------------- the host build
_p, _i, _ll = C.c_void_p, C.c_int, C.c_longlong
SIZES_ARGS = [_p, _i] + [_p] * 6
GRAPHS_ARGS = [_p, _i, _p, _p, _p, _p, _i] + [_p] * 9


def declare(lib):
    lib.ige_create.restype = _p
    lib.ige_create.argtypes = [_i, _p, _p, _p, _p, _i]
    lib.ige_destroy.restype = None
    lib.ige_destroy.argtypes = [_p]
    lib.ige_last_error.restype = C.c_char_p
    lib.ige_last_error.argtypes = [_p]
    lib.ige_invalidate.restype = None
    lib.ige_invalidate.argtypes = [_p]
    lib.ige_chunk.restype = _i
    lib.ige_chunk.argtypes = [_i, _ll, _i]
    lib.ige_sizes.restype = _i
    lib.ige_sizes.argtypes = SIZES_ARGS
    lib.ige_graphs.restype = _i
    lib.ige_graphs.argtypes = GRAPHS_ARGS
    return lib


_emu = []


def emu():
    """tests/hostemu/induced_graph_emu.cpp against csrc/induced_graph_core.h, rebuilt when a source changes"""
    if not _emu:
        so = build_library(os.path.join(hostemu_lib.HOSTEMU, "libinducedgraphemu.so"), hostemu_lib.sources([("induced_graph_emu.cpp", [])]),
                           flags=hostemu_lib.FLAGS)
        _emu.append(declare(C.CDLL(so)))
    return _emu[0]


class EmuInduced:
    """``induced_query_graphs`` with the signature of ``scene.DeviceScene`` through the host build, on a region graph handed in, the
    lanes run forwards or (``backwards``) the other way; a status other than 0 raises ``query_graph_cases.EmuError``"""

    def __init__(self, P, row_ptr, tail, head, rev, backwards=False, lib=None):
        self.lib = lib or emu()
        self.P = P
        self.arrays = [np.ascontiguousarray(row_ptr, np.int64)] + [np.ascontiguousarray(a, np.int32) for a in (tail, head, rev)]
        self.h = self.lib.ige_create(P, *(a.ctypes.data for a in self.arrays), int(backwards))

    def close(self):
        if self.h:
            self.lib.ige_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def error(self):
        return self.lib.ige_last_error(self.h).decode()

    def check(self, rc):
        if rc:
            raise Q.EmuError(rc, self.error())

    def invalidate(self):
        self.lib.ige_invalidate(self.h)

    def raw_sizes(self, *a):
        return self.lib.ige_sizes(self.h, *a)

    def raw_graphs(self, *a):
        return self.lib.ige_graphs(self.h, *a)

    def induced_sizes(self, keep, term_ptr, term_region, st_adjacent):
        return induced_size_arrays(self.P, keep, term_ptr, term_region, st_adjacent, lambda *a: self.check(self.raw_sizes(*a)))[4:]

    def induced_query_graphs(self, keep, term_ptr, term_region, st_adjacent, chunk_queries=0):
        return induced_query_graph_views(self.P, keep, term_ptr, term_region, st_adjacent, lambda *a: self.check(self.raw_sizes(*a)),
                                         lambda *a: self.check(self.raw_graphs(*a)), chunk_queries)


def emu_of(name, backwards=False, lib=None):
    return EmuInduced(*region_graph(name), backwards=backwards, lib=lib)


# ------------------------------------------------------------------------------------------- refusals
FILL = -3


def raw_outputs(num_kept, num_edges):
    """(vertex_off, edge_off, the seven flat output arrays filled with a value no entry takes) for the sizes of a call"""
    B = len(num_kept)
    v = np.zeros(B + 1, np.int64); e = np.zeros(B + 1, np.int64)
    v[1:] = np.cumsum(num_kept.astype(np.int64) + 3); e[1:] = np.cumsum(num_edges)
    V, E = int(v[-1]), int(e[-1])
    return v, e, [np.full(max(s, 1), FILL, np.int32) for s in (E, E, V, 2 * E, 2 * E, E, E)]


def graphs_args(a, outs):
    """the arguments of a raw graphs call behind the handle, from a dict of ``refusals`` and seven output arrays (None: a null one)"""
    at = lambda x: None if x is None else x.ctypes.data
    return (a["B"], at(a["keep"]), at(a["ptr"]), at(a["reg"]), at(a["st"]), a["chunk"], at(a["voff"]), at(a["eoff"])) + tuple(at(o) for o in outs)


def sizes_args(a, num_kept, num_edges):
    at = lambda x: None if x is None else x.ctypes.data
    return a["B"], at(a["keep"]), at(a["ptr"]), at(a["reg"]), at(a["st"]), at(num_kept), at(num_edges)


def refusals(P, keep, ptr, reg, st, voff, eoff):
    """(label, status, text, call 'both' or 'graphs', arguments) for every refusal the header lists, made from a valid call: everything
    ``query_graph_cases.refusals`` changes in the hit lists, and what is new here; needs B >= 2 and a first list of two regions"""
    B = len(st)
    ok = dict(B=B, keep=keep, ptr=ptr, reg=reg, st=st, chunk=0, voff=voff, eoff=eoff)
    cases = []
    for label, status, text, a in Q.refusals(P, 0, ptr, reg, st):
        if "edge_off" in label:
            continue
        cases.append((label, status, text, "graphs" if label == "negative chunk" else "both",
                      dict(ok, B=a["B"], ptr=a["ptr"], reg=a["reg"], st=a["st"], chunk=a["chunk"])))
    dropped = keep.copy(); dropped[1, reg[ptr[1]]] = 0                  # the first hit of query 1's start
    v_short = voff.copy(); v_short[2:] -= 1
    e_long = eoff.copy(); e_long[1:] += 2
    v_low = voff - 1 - voff[0]
    cases += [("hit region not kept", BAD_ARG, r"query 1: hit region \d+ is not kept", "both", dict(ok, keep=dropped)),
              ("null keep", BAD_ARG, "null", "both", dict(ok, keep=None)),
              ("null st_adjacent", BAD_ARG, "null", "both", dict(ok, st=None)),
              ("null vertex_off", BAD_ARG, "null", "graphs", dict(ok, voff=None)),
              ("null edge_off", BAD_ARG, "null", "graphs", dict(ok, eoff=None)),
              ("vertex_off one short", BAD_ARG, "vertex_off of query 1", "graphs", dict(ok, voff=v_short)),
              ("edge_off two long", BAD_ARG, "edge_off of query 0", "graphs", dict(ok, eoff=e_long)),
              ("vertex_off from below 0", BAD_ARG, "starts below 0", "graphs", dict(ok, voff=v_low))]
    return cases


def check_refusals(raw_sizes, raw_graphs, last_error, name="boxes130", B=5):
    """every refusal of induced_graph_cases.refusals through the raw calls ``raw_sizes(*arguments)`` / ``raw_graphs(*arguments)``:
    the status, the text, outputs read back as they were filled, and a valid call afterwards with the bytes of the one before"""
    P = region_graph(name)[0]
    keep, ptr, reg, st = batch(name, B, "random0.5", seed=1)               # (the first list has two regions)
    ref = reference(name, keep, ptr, reg, st)
    num_kept, num_edges = reference_sizes(ref)
    voff, eoff, outs = raw_outputs(num_kept, num_edges)
    ok = dict(B=B, keep=keep, ptr=ptr, reg=reg, st=st, chunk=0, voff=voff, eoff=eoff)
    assert raw_graphs(*graphs_args(ok, outs)) == OK and not any(np.any(o == FILL) for o in outs)
    first = [o.copy() for o in outs]
    cases = refusals(P, keep, ptr, reg, st, voff, eoff)
    assert len(cases) >= 18
    for label, status, text, which, a in cases:
        _, _, outs = raw_outputs(num_kept, num_edges)
        assert raw_graphs(*graphs_args(a, outs)) == status, label
        assert re.search(text, last_error()), (label, last_error())
        assert all(np.all(o == FILL) for o in outs), label
        if which == "both":
            kept, edges = np.full(B, FILL, np.int32), np.full(B, FILL, np.int64)
            assert raw_sizes(*sizes_args(a, kept, edges)) == status, label
            assert re.search(text, last_error()), (label, last_error())
            assert np.all(kept == FILL) and np.all(edges == FILL), label
    for k in range(7):                                                       # a null output array
        _, _, outs = raw_outputs(num_kept, num_edges)
        holed = [None if j == k else o for j, o in enumerate(outs)]
        assert raw_graphs(*graphs_args(ok, holed)) == BAD_ARG and re.search("null", last_error()), k
        assert all(np.all(o == FILL) for o in outs), k
    kept = np.full(B, FILL, np.int32)
    assert raw_sizes(*sizes_args(ok, kept, None)) == BAD_ARG and np.all(kept == FILL)
    _, _, outs = raw_outputs(num_kept, num_edges)
    assert raw_graphs(*graphs_args(ok, outs)) == OK
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, first))


# ------------------------------------------------------------------------------------------- whole graphs
FIELDS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr", "poly_A", "poly_b", "interior")


def assert_same_graph(g, h):
    assert (g.n, g.keys, g.src, g.dst) == (h.n, h.keys, h.src, h.dst) and type(g.keys) is list
    for f in FIELDS:
        a, b = getattr(g, f), getattr(h, f)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f
