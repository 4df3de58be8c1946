"""The candidate paths of the rounding step drawn on the device: the host side of ``gcsadmm_walks_*`` (include/gcsadmm.h) and the
rule they follow, restated in plain Python.

``rounding.rounding`` walks the relaxed edge activations on the host, from dictionaries with one entry per edge and with all draws
of a problem taken from one sequential generator.  For a batch of queries that is the only work per edge left between the stop test
and the final path.  ``DeviceWalks`` keeps the out-lists of many problems on the device and draws their walks there, reading every
problem's activations where the solver left them; the draws come from a counter-based generator, so every (problem, walk) pair is
independent of every other.  The rule is new -- it does not reproduce the host generator's draws -- and ``walk_reference`` below is
its definition: csrc/path_walk_core.h states the same rule, and the kernel and its host build are held to this function element for
element.  There is no CPU fallback: ``walk_reference`` is the specification and a test's sampler, not a product path.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import abi
from .abi import GcsAdmmError

__all__ = ["out_lists", "walk_reference", "DeviceWalks", "OK", "DEAD_END", "TOO_LONG", "MAX_VERTICES", "MAX_DEGREE"]

OK, DEAD_END, TOO_LONG = 0, 1, 2
MAX_VERTICES = 524288       # the visited bitmap of one problem is 64 KB of LDS
MAX_DEGREE = 1 << 22        # 2^22 weights of at most 2^41: a total stays within 64 bits
_MASK = (1 << 64) - 1


def out_lists(g):
    """``(out_ptr, out_head, out_edge)`` of a ``GcsGraph``, int32: the out-list of vertex v is ``out_ptr[v]:out_ptr[v + 1]``, in edge
    order (a stable sort of the edges by tail: the order of ``rounding_problem``'s ``I_v_out``); ``out_head[k]`` is the head vertex
    and ``out_edge[k]`` the edge, which indexes the activations."""
    tail = np.asarray(g.edge_tail, np.int64)
    order = np.argsort(tail, kind="stable")
    out_ptr = np.zeros(g.num_vertices + 1, np.int64)
    out_ptr[1:] = np.cumsum(np.bincount(tail, minlength=g.num_vertices))
    return out_ptr.astype(np.int32), np.asarray(g.edge_head, np.int32)[order], order.astype(np.int32)


def weight(y) -> int:
    """the exact integer weight of an activation: 0 unless y > 0, else floor(min(y, 2) * 2^40), y widened to double first"""
    y = float(y)
    if not y > 0.0:
        return 0
    return int(math.floor(min(y, 2.0) * 2.0 ** 40))


def mix(seed: int, walk: int, j: int) -> int:
    """splitmix64 on the counter ``(walk << 32) + j + 1``"""
    z = (seed + 0x9E3779B97F4A7C15 * ((walk << 32) + j + 1)) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def walk_reference(out_ptr, out_head, out_edge, y, src, dst, seed, walk, max_len):
    """Walk number ``walk`` of one problem under the activations ``y`` (by edge id; float64 or float32), ``(path, status)``: the
    vertices from ``src`` as an int32 array and OK (reached ``dst``), DEAD_END or TOO_LONG.  Python integers throughout.

    At vertex v, position j of the path (``src`` is position 0): the weight of out-list entry k is ``weight(y[out_edge[k]])``, 0 when
    its head is on the path already; ``tot`` is their sum.  ``tot == 0``: a dead end, the path so far is kept.  A path of ``max_len``
    vertices that is not at ``dst`` and not at a dead end: TOO_LONG.  Walk 0 takes the entry of largest weight, among equals the last;
    walk w >= 1 takes the first entry whose inclusive prefix sum exceeds ``(mix(seed, w, j) * tot) >> 64``."""
    seed = int(seed) & _MASK
    path, visited, cur = [int(src)], {int(src)}, int(src)
    while cur != dst:
        ks = range(int(out_ptr[cur]), int(out_ptr[cur + 1]))
        ws = [0 if int(out_head[k]) in visited else weight(y[out_edge[k]]) for k in ks]
        tot = sum(ws)
        if tot == 0:
            return np.array(path, np.int32), DEAD_END
        if len(path) == max_len:
            return np.array(path, np.int32), TOO_LONG
        if walk == 0:
            pick = max((w, k) for w, k in zip(ws, ks))[1]
        else:
            r = (mix(seed, walk, len(path) - 1) * tot) >> 64
            acc = 0
            for w, k in zip(ws, ks):
                acc += w
                if acc > r:
                    pick = k
                    break
        cur = int(out_head[pick])
        visited.add(cur); path.append(cur)
    return np.array(path, np.int32), OK


class DeviceWalks:
    """The out-lists of many problems resident on the device (``gcsadmm_walks_create``): ``graphs`` are ``GcsGraph`` instances, or
    tuples ``(out_ptr, out_head, out_edge, src, dst)`` of a problem that has no region graph.  More than 524 288 vertices in one
    problem or an out-degree above 2^22 is refused.  Release with ``close()`` or use as a context manager.  There is no CPU fallback."""

    def __init__(self, graphs, device: int = 0):
        self.lib = abi.load_library()
        self.device = int(device)
        self._h = C.c_void_p()
        lists = [tuple(g) if isinstance(g, (tuple, list)) else (*out_lists(g), g.src, g.dst) for g in graphs]
        self.B = len(lists)
        self.num_vertices = [len(l[0]) - 1 for l in lists]
        self.num_edges = [len(l[1]) for l in lists]
        i32 = lambda parts: np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32).ravel() for p in parts]) if parts else np.zeros(0), np.int32)
        vertex_off = np.zeros(self.B + 1, np.int64); vertex_off[1:] = np.cumsum(self.num_vertices)
        edge_off = np.zeros(self.B + 1, np.int64); edge_off[1:] = np.cumsum(self.num_edges)
        for i, l in enumerate(lists):
            if len(l[0]) < 1 or len(l[2]) != len(l[1]):
                raise ValueError(f"problem {i}: out_ptr needs V + 1 entries, out_head and out_edge one per edge")
        out_ptr, out_head, out_edge = (i32([l[f] for l in lists]) for f in range(3))
        src, dst = i32([[l[3]] for l in lists]), i32([[l[4]] for l in lists])
        h = C.c_void_p()
        st = self.lib.gcsadmm_walks_create(self.B, vertex_off.ctypes.data, edge_off.ctypes.data, out_ptr.ctypes.data, out_head.ctypes.data,
                                           out_edge.ctypes.data, src.ctypes.data, dst.ctypes.data, self.device, C.byref(h))
        abi.check(st, lambda: f"gcsadmm_walks_create failed (status {st}): {self.lib.gcsadmm_walks_last_error(None).decode()}")
        self._h = h

    def _call(self, name, *args):
        if not self._h:
            raise GcsAdmmError("the walks object is closed")
        st = getattr(self.lib, name)(self._h, *args)
        abi.check(st, lambda: f"{name} failed (status {st}): {self.lib.gcsadmm_walks_last_error(self._h).decode()}")

    def close(self):
        if self._h:
            self._call("gcsadmm_walks_destroy")
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sample(self, y, seeds, first: int = 0, count: int = 21, max_len=None):
        """Walks ``first .. first + count - 1`` of every problem.  ``y``: one contiguous device tensor per problem with its activations by
        edge id (``member.zedge[2 * n]``), all float64 or all float32; ``seeds``: one integer per problem (taken modulo 2^64);
        ``max_len``: the most vertices of a path (default: those of the largest problem, which no simple path exceeds).  Enqueued on
        the current stream, behind the work that wrote ``y``.  Returns one ``(paths, status)`` per problem: ``count`` int32 arrays of
        vertex ids and the int32 array of their statuses (OK, DEAD_END, TOO_LONG); a path that did not reach ``dst`` is what was
        walked of it."""
        import torch
        if len(y) != self.B or len(seeds) != self.B:
            raise ValueError("one activation tensor and one seed per problem")
        if max_len is None:
            max_len = max(self.num_vertices, default=1)
        dtypes = {t.dtype for t in y}
        if len(dtypes) > 1 or (dtypes and dtypes not in ({torch.float64}, {torch.float32})):
            raise ValueError("the activations must be all float64 or all float32")
        for i, t in enumerate(y):
            if not t.is_cuda or t.device.index != self.device or not t.is_contiguous() or t.numel() < self.num_edges[i]:
                raise ValueError(f"problem {i}: the activations must be a contiguous tensor of {self.num_edges[i]} entries on device {self.device}")
        dtype = abi.F32 if dtypes == {torch.float32} else abi.F64
        ptrs = (C.c_void_p * max(self.B, 1))(*[t.data_ptr() for t in y])
        seed = np.array([((int(s) & _MASK) ^ (1 << 63)) - (1 << 63) for s in seeds], np.int64)      # the same 64 bits, as int64
        count, max_len = int(count), int(max_len)
        cells = max(self.B * count * max_len, 0) if count > 0 and max_len > 0 else 0
        vtx = np.zeros(cells if cells <= 2 ** 31 - 1 else 0, np.int32)
        length = np.zeros(self.B * max(count, 0), np.int32); status = np.zeros(self.B * max(count, 0), np.int32)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self._call("gcsadmm_walks_sample", ptrs, dtype, seed.ctypes.data, int(first), count, max_len, stream, vtx.ctypes.data,
                       length.ctypes.data, status.ctypes.data)
        vtx = vtx.reshape(self.B, count, max_len) if cells else vtx
        length, status = length.reshape(self.B, count), status.reshape(self.B, count)
        return [([vtx[i, w, :length[i, w]].copy() for w in range(count)], status[i].copy()) for i in range(self.B)]
