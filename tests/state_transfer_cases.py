"""Graphs, states, the host build and the reference for the tests of the state transfer (csrc/state_transfer_core.h;
gcsadmm_export_state / gcsadmm_import_state and their batch forms in csrc/gcsadmm.hip), shared by test_state_transfer.py (host build,
no GPU) and test_gpu_state_transfer.py.

A ``Side`` is one member as the transfer sees it: a graph, its vertex ids, its column numbering and state type, its six state arrays and
its control block's rho and mu_scale.  Reference: ``transfer_reference``, a restatement in plain numpy by dictionaries of keys -- no
search, no code shared with the header --, compared by dtype, shape and bytes; no tolerance anywhere."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import hostemu_lib
from gcs_admm_amd import abi
from gcs_admm_amd.graph import _finish_graph
from gcs_admm_amd.native_build import build_library

EMU_SRC = os.path.join(hostemu_lib.HOSTEMU, "state_transfer_emu.cpp")
OK, BAD_ARG = 0, 1
STATE = ("copy", "mu", "zedge", "xv", "zv", "yv")
SNAPSHOT = ("edge_key", "edge_words", "vertex_id", "vertex_words", "rho")
NP_DTYPE = {"f64": np.float64, "f32": np.float32}
ID_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------- graphs
def graph_of(n, V, tail, head):
    """a GcsGraph on vertices 0 (the start) .. V-1 with the edge list given: unit boxes in a row, the two terminals point boxes"""
    lo = np.zeros((V, n)); lo[:, 0] = 2.0 * np.arange(V)
    hi = lo + 1.0
    cen = 0.5 * (lo + hi)
    for t in (0, 1):
        lo[t], hi[t] = cen[t] - 1e-6, cen[t] + 1e-6
    A = np.vstack([np.eye(n), -np.eye(n)])
    polys = [(A, np.hstack([hi[v], -lo[v]])) for v in range(V)]
    return _finish_graph(n, ['s', 't'] + list(range(V - 2)), np.asarray(tail, np.int32), np.asarray(head, np.int32), polys, cen, 0, 1)


def random_edges(V, E, rng):
    """E distinct edges (u, w), u != w, strictly ascending in (tail, head)"""
    assert E <= V * (V - 1)
    code = np.sort(rng.choice(V * (V - 1), size=E, replace=False))
    u, k = code // (V - 1), code % (V - 1)
    return u.astype(np.int32), (k + (k >= u)).astype(np.int32)


def vertices_for(E):
    """a vertex count for E random edges: mean degree about 12, at least 4"""
    return max(4, int(np.ceil(E / 6)) + 2)


class Side:
    """one member: ``g``, ``ids`` int32 [V] ascending, ``columns`` "incidence" | "edge", ``dtype`` "f64" | "f32", the six state arrays
    (``fill``: "random" finite values, "nan", or "zero"), ``rho`` and ``mu_scale`` of its control block"""

    def __init__(self, g, ids, columns="incidence", dtype="f64", fill="random", rho=1.0, mu_scale=1.0, seed=0):
        self.g, self.ids, self.columns, self.dtype = g, np.ascontiguousarray(ids, np.int32), columns, dtype
        self.rho, self.mu_scale = float(rho), float(mu_scale)
        c, E, V, n, T = g.c, g.num_edges, g.num_vertices, g.n, NP_DTYPE[dtype]
        rng = np.random.default_rng(seed)
        shapes = dict(copy=(c, max(2 * E, 1)), mu=(c, max(2 * E, 1)), zedge=(c, max(E, 1)), xv=(V, 2 * n), zv=(V, 2 * n), yv=(V,))
        make = {"random": lambda s, t: rng.standard_normal(s).astype(t), "nan": lambda s, t: np.full(s, np.nan, t),
                "zero": lambda s, t: np.zeros(s, t)}[fill]
        self.state = {k: make(s, T if k in ("copy", "mu", "zedge") else np.float64) for k, s in shapes.items()}

    @property
    def tail_col(self):
        E = self.g.num_edges
        return np.arange(E) if self.columns == "edge" else self.g.edge_inc_tail.astype(np.int64)

    @property
    def head_col(self):
        E = self.g.num_edges
        return E + np.arange(E) if self.columns == "edge" else self.g.edge_inc_head.astype(np.int64)

    def with_state(self, state):
        s = Side.__new__(Side)
        s.__dict__.update(self.__dict__)
        s.state = {k: v.copy() for k, v in state.items()}
        return s


def side(n, E, ids=None, V=None, seed=0, **kw):
    """a Side on E random edges (V vertices, default ``vertices_for(E)``; ``ids``: default 0, 1, 3, 5, ..)"""
    V = V or vertices_for(E)
    rng = np.random.default_rng(1000 * E + n + seed)
    tail, head = random_edges(V, E, rng)
    if ids is None:
        ids = np.concatenate([[0, 1], 3 + 2 * np.arange(V - 2)])
    return Side(graph_of(n, V, tail, head), ids, seed=seed + 1, **kw)


def subgraph_side(src, keep_vertices, extra_edges=(), seed=0, **kw):
    """a Side on the vertices ``keep_vertices`` of ``src`` (a bool mask; the terminals stay) with the induced edges, the ids carried
    along; ``extra_edges``: pairs of NEW vertex indices added to the list (edges the source does not have)"""
    g = src.g
    keep = np.asarray(keep_vertices, bool).copy(); keep[:2] = True
    new = np.cumsum(keep) - 1
    both = keep[g.edge_tail] & keep[g.edge_head]
    pairs = {(int(new[u]), int(new[w])) for u, w in zip(g.edge_tail[both], g.edge_head[both])} | {(int(u), int(w)) for u, w in extra_edges}
    pairs = sorted(pairs)
    tail, head = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    return Side(graph_of(g.n, int(keep.sum()), tail, head), src.ids[keep], seed=seed + 7, **kw)


# ------------------------------------------------------------------------------------------- the reference
def _key(ids, u, w):
    return (int(ids[u]) << 32) | int(ids[w])


def export_reference(src):
    """the five arrays of the snapshot ``src`` exports, sized exactly V and E"""
    g, st, T = src.g, src.state, NP_DTYPE[src.dtype]
    c, E, V, n = g.c, g.num_edges, g.num_vertices, g.n
    ms = np.float64(src.mu_scale)
    ct, ch = src.tail_col, src.head_col
    words = np.zeros((5, c, E), T)
    words[0] = st["zedge"][:, :E]
    words[1], words[2] = st["copy"][:, ct], st["copy"][:, ch]
    words[3] = (ms * st["mu"][:, ct].astype(np.float64)).astype(T)
    words[4] = (ms * st["mu"][:, ch].astype(np.float64)).astype(T)
    vw = np.concatenate([st["xv"].T, st["zv"].T, st["yv"][None]]).astype(np.float64)
    return dict(edge_key=np.array([_key(src.ids, u, w) for u, w in zip(g.edge_tail, g.edge_head)], np.int64).reshape(E),
                edge_words=words, vertex_id=src.ids.copy(), vertex_words=np.ascontiguousarray(vw).reshape(4 * n + 1, V),
                rho=np.array([src.rho]))


def transfer_reference(src, dst):
    """the six state arrays of ``dst`` after importing what ``src`` exports: by dictionaries of edge keys and vertex ids.  A matched
    mu word is T(f64(T(mu_scale * f64(mu))) * (rho_src / rho_dst)); everything else a copy; what is not matched is zero."""
    gs, gd, T = src.g, dst.g, NP_DTYPE[dst.dtype]
    assert src.dtype == dst.dtype and gs.n == gd.n
    ss = src.state
    ms, r = np.float64(src.mu_scale), np.float64(src.rho) / np.float64(dst.rho)
    edges, vertices = {}, {}
    for e, (u, w, a, b) in enumerate(zip(gs.edge_tail, gs.edge_head, src.tail_col, src.head_col)):
        edges[_key(src.ids, u, w)] = (ss["zedge"][:, e], ss["copy"][:, a], ss["copy"][:, b],
                                      (ms * ss["mu"][:, a].astype(np.float64)).astype(T), (ms * ss["mu"][:, b].astype(np.float64)).astype(T))
    for v in range(gs.num_vertices):
        vertices[int(src.ids[v])] = (ss["xv"][v], ss["zv"][v], ss["yv"][v])
    out = {k: np.zeros_like(a) for k, a in dst.state.items()}
    for e, (u, w, a, b) in enumerate(zip(gd.edge_tail, gd.edge_head, dst.tail_col, dst.head_col)):
        hit = edges.get(_key(dst.ids, u, w))
        if hit is not None:
            out["zedge"][:, e], out["copy"][:, a], out["copy"][:, b] = hit[0], hit[1], hit[2]
            out["mu"][:, a] = (hit[3].astype(np.float64) * r).astype(T)
            out["mu"][:, b] = (hit[4].astype(np.float64) * r).astype(T)
    for v in range(gd.num_vertices):
        hit = vertices.get(int(dst.ids[v]))
        if hit is not None:
            out["xv"][v], out["zv"][v], out["yv"][v] = hit
    if gd.num_edges == 0:       # the one padding column of an empty member is not the transfer's
        for k in ("copy", "mu", "zedge"):
            out[k] = dst.state[k].copy()
    return out


def same_state(got, want, label=""):
    for k in STATE:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (label, k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (label, k, np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))[:5].tolist())


def same_snapshot(got, want, label=""):
    """``got``: the arrays of a snapshot with room for at least (V, E); the first V / E entries, at the strides V / E, are the export"""
    E, V = want["edge_key"].shape[0], want["vertex_id"].shape[0]
    for k in SNAPSHOT:
        a = got[k].ravel()[:want[k].size].reshape(want[k].shape)
        assert a.dtype == want[k].dtype, (label, k, a.dtype)
        assert a.tobytes() == want[k].tobytes(), (label, k)
    assert (got["V"], got["E"]) == (V, E), label


# ------------------------------------------------------------------------------------------- snapshots
class SnapshotArrays:
    """host arrays of a snapshot with room for (V, E), every entry a value no export writes, and its gcsadmm_snapshot"""

    def __init__(self, n, dtype, V, E):
        T = NP_DTYPE[dtype]
        self.n, self.dtype = n, dtype
        self.arrays = dict(edge_key=np.full(max(E, 1), -5, np.int64), edge_words=np.full(5 * (2 * n + 1) * max(E, 1), np.nan, T),
                           vertex_id=np.full(max(V, 1), -5, np.int32), vertex_words=np.full((4 * n + 1) * max(V, 1), np.nan), rho=np.full(1, np.nan))
        self.c = abi.Snapshot(n=n, state_dtype=abi.F64 if dtype == "f64" else abi.F32, V=V, E=E, **{k: a.ctypes.data for k, a in self.arrays.items()})

    def read(self):
        return dict(self.arrays, V=self.c.V, E=self.c.E)


def snapshot_for(s, slack=0):
    return SnapshotArrays(s.g.n, s.dtype, s.g.num_vertices + slack, s.g.num_edges + slack)


# ------------------------------------------------------------------------------------------- the host build
_p, _i, _d = C.c_void_p, C.c_int, C.c_double


def declare(lib):
    lib.ste_create.restype, lib.ste_create.argtypes = _p, [_i] * 6 + [_p] * 4
    lib.ste_destroy.restype, lib.ste_destroy.argtypes = None, [_p]
    lib.ste_reset.restype, lib.ste_reset.argtypes = None, [_p, _d, _d]
    lib.ste_last_error.restype, lib.ste_last_error.argtypes = C.c_char_p, []
    lib.ste_transfer.restype, lib.ste_transfer.argtypes = _i, [_i, _p, _p, _p, _p, _i, _i, _i]
    return lib


EMU_FLAGS = hostemu_lib.FLAGS + [hostemu_lib.INCLUDE]
_emu = []


def emu():
    """tests/hostemu/state_transfer_emu.cpp against csrc/state_transfer_core.h, rebuilt when a source changes"""
    if not _emu:
        so = build_library(os.path.join(hostemu_lib.HOSTEMU, "libstatetransferemu.so"), [(EMU_SRC, [])], flags=EMU_FLAGS)
        _emu.append(declare(C.CDLL(so)))
    return _emu[0]


class EmuMember:
    """a Side behind the host build: its handle stand-in and a gcsadmm_state on the Side's own arrays (an import writes into them)"""

    def __init__(self, s, lib=None, reset=True, num_incidences=None):
        self.lib, self.side = lib or emu(), s
        g = s.g
        E = g.num_edges
        self.keep = [np.ascontiguousarray(a, np.int32) for a in (g.edge_tail, g.edge_head, s.tail_col, s.head_col)]
        self.h = self.lib.ste_create(g.n, abi.F64 if s.dtype == "f64" else abi.F32, g.num_vertices, E, 2 * E if num_incidences is None else num_incidences,
                                     int(s.columns == "edge"), *(a.ctypes.data for a in self.keep))
        if reset:
            self.lib.ste_reset(self.h, s.rho, s.mu_scale)
        self.c_state = abi.State(*(s.state[k].ctypes.data for k in STATE))

    def close(self):
        if self.h:
            self.lib.ste_destroy(self.h)
            self.h = None


def emu_call(members, snapshots, exporting, solo=False, backwards=False, lib=None, ids=None, states=None):
    """one call of the host build: ``members`` [EmuMember], ``snapshots`` [SnapshotArrays or None]; returns (status, text)"""
    lib = lib or emu()
    n = len(members)
    handles = (C.c_void_p * n)(*[m.h for m in members])
    st = (abi.State * n)(*[m.c_state for m in members]) if states is None else states
    id_arrays = [m.side.ids for m in members] if ids is None else ids
    idp = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in id_arrays])
    snp = (C.c_void_p * n)(*[None if s is None else C.addressof(s.c) for s in snapshots])
    rc = lib.ste_transfer(n, handles, st, idp, snp, int(exporting), int(solo), int(backwards))
    return rc, lib.ste_last_error().decode()


def emu_transfer(src, dst, backwards=False, lib=None, slack=0):
    """export ``src``, import into ``dst`` through the host build, one solo call each: (the snapshot's arrays, dst's state after)"""
    a, b = EmuMember(src, lib), EmuMember(dst.with_state(dst.state), lib)
    try:
        snap = snapshot_for(src, slack)
        rc, text = emu_call([a], [snap], True, solo=True, backwards=backwards, lib=lib)
        assert rc == OK, text
        rc, text = emu_call([b], [snap], False, solo=True, backwards=backwards, lib=lib)
        assert rc == OK, text
        return snap.read(), b.side.state
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------- the tables (host build and device)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257)      # source E: one lane, the tile of 64 x 4 lanes and its neighbours, more than one workgroup
DIMS = (1, 2, 3, 8)                            # c = 3, 5, 7, 17


def round_trip_cases():
    """(label, Side) for export then import on the same graph: every n, both state types, both numberings"""
    for n in DIMS:
        for dtype in ("f64", "f32"):
            for columns in ("incidence", "edge"):
                # (40 vertices: degrees small enough for the n = 8 sub-problems to fit a CU's LDS when the device runs the table)
                yield f"n{n}-{dtype}-{columns}", side(n, 37 + 3 * n, V=40, columns=columns, dtype=dtype, seed=n)


def pair_cases(n=2, dtype="f64", columns=("incidence", "edge")):
    """(label, source Side, destination Side) of the different-graph table; the destination arrives filled with NaN"""
    cs, cd = columns
    big = 10 ** 9
    for E in SIZES:
        src = side(n, E, columns=cs, dtype=dtype, seed=E)
        V = src.g.num_vertices
        yield f"same-E{E}", src, Side(src.g, src.ids, cd, dtype, fill="nan")
        drop = np.ones(V, bool); drop[2::3] = False
        yield f"pruned-E{E}", src, subgraph_side(src, drop, columns=cd, dtype=dtype, fill="nan")
    src = side(n, 90, columns=cs, dtype=dtype, seed=5)
    V = src.g.num_vertices
    # a superset: the source is the pruned one
    some = np.ones(V, bool); some[3::2] = False
    yield "superset", subgraph_side(src, some, columns=cs, dtype=dtype), Side(src.g, src.ids, cd, dtype, fill="nan")
    yield "disjoint", src, Side(src.g, src.ids + 2 * V + 7, cd, dtype, fill="nan")
    yield "source-without-edges", Side(graph_of(n, 4, [], []), [0, 1, 5, 9], cs, dtype), side(n, 9, ids=[0, 1, 5, 9], V=4, columns=cd, dtype=dtype, fill="nan")
    yield "destination-without-edges", src, Side(graph_of(n, V, [], []), src.ids, cd, dtype, fill="nan")
    # ids up to 2^31 - 1: keys that agree in their low or in their high 32 bits
    ids = np.array([0, 1, 2, 2 ** 16, 2 ** 31 - 2, ID_MAX], np.int32)
    hsrc = Side(graph_of(n, 6, [2, 2, 3, 4, 5, 5], [3, 5, 5, 2, 2, 4]), ids, cs, dtype, seed=3)
    yield "high-ids", hsrc, Side(graph_of(n, 6, [2, 3, 3, 4, 5, 5], [5, 2, 5, 5, 3, 4]), ids, cd, dtype, fill="nan")
    # terminal edges on one side only, and an s-t edge
    t = side(n, 30, V=8, columns=cs, dtype=dtype, seed=9)
    inner = {(int(u), int(w)) for u, w in zip(t.g.edge_tail, t.g.edge_head) if min(u, w) >= 2}
    with_ends = lambda extra, **kw: Side(graph_of(n, 8, *zip(*sorted(inner | set(extra)))), t.ids, dtype=dtype, **kw)
    yield "terminal-edges", with_ends([(0, 2), (2, 0), (0, 1), (1, 4), (4, 1)], columns=cs, seed=11), \
        with_ends([(1, 3), (3, 1), (1, 0), (1, 4), (4, 1)], columns=cd, fill="nan")


def neighbour_key_cases(n=2, dtype="f64"):
    """every destination key just below, at and just above every source key: a chain whose ids step by 2, so that id +- 1 is free"""
    V = 12
    ids = np.concatenate([[0, 1], 10 + 4 * np.arange(V - 2)]).astype(np.int32)
    tail = np.arange(2, V - 1, dtype=np.int32); head = tail + 1
    src = Side(graph_of(n, V, tail, head), ids, "incidence", dtype, seed=2)
    yield "at", src, Side(src.g, ids, "edge", dtype, fill="nan")
    for name, d_tail, d_head in (("head-1", 0, -1), ("head+1", 0, 1), ("tail-1", -1, 0), ("tail+1", 1, 0)):
        # vertex v keeps its id as a tail when d_tail == 0; a shifted copy of every vertex is added beside it
        both = np.sort(np.concatenate([ids, ids[2:] + (d_tail or d_head)])).astype(np.int32)
        pos = {int(i): k for k, i in enumerate(both)}
        t2 = np.array([pos[int(ids[u]) + d_tail] for u in tail], np.int32); h2 = np.array([pos[int(ids[w]) + d_head] for w in head], np.int32)
        o = np.lexsort((h2, t2))
        yield name, src, Side(graph_of(n, len(both), t2[o], h2[o]), both, "edge", dtype, fill="nan")
