"""Many small problems in one set of launches: the host side of the batch entry points of include/gcsadmm.h.

A small graph leaves most of an MI355X idle, and its vertex step is bound by dependent latency, so users with many small problems
(many start / goal queries, many scenes) gain from occupancy: ``BatchSolver`` holds one ordinary ``DeviceSolver`` per graph and
advances all of them with one vertex launch and one edge + control launch per iteration.  Every member keeps its own state, control
block and trace, stops on its own, and computes bit for bit what the same solver computes when it is driven alone.

``large=True`` (GCSADMM_BATCH_LARGE of include/gcsadmm.h) also takes the graphs a plain batch refuses: members on the wavefront program,
whose launch fills a fraction of the chip's 1 024 wavefront slots once it packs several vertices per wavefront, and members of 512 or
more workgroup-program vertices.  ``member_programs`` is the rule that chooses each member's program.

``region_terminals=True`` (GCSADMM_BATCH_TERMINALS) takes members whose start or goal is a set with an extent: their terminals are
solved in one launch per group of terminals (thread count, home of the work arrays) beside the vertex launches.  It is opt-in and may
be combined with ``large``.
"""
from __future__ import annotations

import ctypes as C
import time

from . import abi
from .abi import RUNNING, State
from .solver import DeviceSolver

WAVE_SLOTS_ON_CHIP = 1024      # one wavefront of the wavefront program per SIMD: gcsadmm_create's own crossover between the two programs
WAVE_MAX_SLOTS = 7             # vertices a wavefront may take (gcs::MAX_SLOTS, csrc/vertex_program.inc)
WAVE_MAX_DEGREE = 63           # a vertex and its incident edges fill at most one wavefront


def generic_degrees(g):
    """degrees of the generic vertices of ``g``: those with an interior-point solve (not a terminal, edges in and out)"""
    import numpy as np
    deg = np.diff(np.asarray(g.inc_ptr)).astype(np.int64)
    out = np.add.reduceat(np.append(np.asarray(g.inc_out, dtype=np.int64), 0), np.asarray(g.inc_ptr[:-1], dtype=np.int64)) * (deg > 0)
    keep = (out > 0) & (deg - out > 0)
    keep[[v for v in (g.src, g.dst) if 0 <= v < len(keep)]] = False
    return deg[keep]


def member_programs(graphs, large: bool = False):
    """The ``DeviceSolver`` knobs of every member of a batch over ``graphs``, one dict each.

    Plain batch: ``program="workgroup256"`` for all.  ``large``: at n = 2, when the generic vertices of the WHOLE batch exceed 1 024,
    the members whose generic vertices all have degree <= 63 run ``program="wavefront"`` with ``wave_slots = min(7, ceil(total generic
    / 1024))``; every other member stays on ``"workgroup256"``.  1 024 is gcsadmm_create's crossover between the two programs (one
    round of the workgroup program at four workgroups per CU; the wavefront program's slots on the chip) and the slot count its packing
    rule, both applied to the batch as a whole instead of to one graph: the launches of a batch hold all members at once."""
    plain = [dict(program="workgroup256") for _ in graphs]
    if not large or not graphs or any(g.n != 2 for g in graphs):
        return plain
    degrees = [generic_degrees(g) for g in graphs]
    total = int(sum(len(d) for d in degrees))
    if total <= WAVE_SLOTS_ON_CHIP:
        return plain
    slots = min(WAVE_MAX_SLOTS, -(-total // WAVE_SLOTS_ON_CHIP))
    return [dict(program="wavefront", wave_slots=slots) if len(d) and d.max() <= WAVE_MAX_DEGREE else k for d, k in zip(degrees, plain)]


class BatchSolver:
    """``graphs``: GcsGraph instances of one space dimension, small enough for the workgroup program (fewer than 512 generic vertices
    each) unless ``large``.  ``members[i]`` is the ``DeviceSolver(graphs[i], **member_programs(graphs, large)[i])`` of graph i
    (``program="workgroup256"`` in a plain batch): its state tensors, ``cost()``, ``read_control()`` and rounding work per member as
    they do for a solver of its own."""

    def __init__(self, graphs, state_dtype: str = "f64", device=None, large: bool = False, region_terminals: bool = False):
        graphs = list(graphs)
        self.members = [DeviceSolver(g, state_dtype, device=device, **knobs) for g, knobs in zip(graphs, member_programs(graphs, large))]
        self.b = None
        self._init(self.members, large, region_terminals)

    @classmethod
    def of(cls, members, large: bool = False, region_terminals: bool = False):
        """a batch over existing solvers (they stay the caller's and must outlive the batch); ``large``: created with
        GCSADMM_BATCH_LARGE, so the solvers may run the wavefront program or hold 512 and more workgroup-program vertices;
        ``region_terminals``: created with GCSADMM_BATCH_TERMINALS, so the solvers may have a terminal that is a region"""
        self = cls.__new__(cls)
        self.members, self.b = list(members), None
        self._init(self.members, large, region_terminals)
        return self

    def _init(self, members, large=False, region_terminals=False):
        import torch
        self.torch, self.lib = torch, abi.load_library()
        self.device = members[0].device if members else torch.device("cuda", torch.cuda.current_device())
        handles = (C.c_void_p * max(len(members), 1))(*[m.h.value for m in members])
        b = C.c_void_p()
        flags = (abi.BATCH_LARGE if large else 0) | (abi.BATCH_TERMINALS if region_terminals else 0)
        if flags:
            self._call("gcsadmm_batch_create_ex", handles, len(members), flags, C.byref(b), batch=False)
        else:
            self._call("gcsadmm_batch_create", handles, len(members), C.byref(b), batch=False)
        self.large, self.region_terminals, self.b = bool(large), bool(region_terminals), b

    # ------------------------------------------------------------------
    def _call(self, name, *args, batch=True):
        """The one call into the library, as DeviceSolver._call: ``name(self.b, *args)`` (``batch=False``: ``name(*args)``, and the error
        text is the calling thread's) with the batch's device current; a status other than 0 raises GcsAdmmError."""
        b = self.b if batch else None
        with self.torch.cuda.device(self.device):
            st = getattr(self.lib, name)(*((b,) if batch else ()), *args)
        abi.check(st, lambda: f"{name} failed ({st}): {self.lib.gcsadmm_batch_last_error(b).decode()}")

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        """destroys the batch; the members stay usable on their own"""
        if getattr(self, "b", None):
            self._call("gcsadmm_batch_destroy")
            self.b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.members)

    def launches(self):
        """(members in the workgroup launch, wave launches, members over all wave launches) of one iteration (gcsadmm_batch_query)"""
        out = [C.c_int32() for _ in range(3)]
        self._call("gcsadmm_batch_query", *[C.byref(o) for o in out])
        return tuple(o.value for o in out)

    def terminal_launches(self):
        """(terminal launches, region terminals over all of them) of one iteration (gcsadmm_batch_query_terminals): (0, 0) unless
        the batch was made with ``region_terminals`` and a member has such a terminal"""
        out = [C.c_int32() for _ in range(2)]
        self._call("gcsadmm_batch_query_terminals", *[C.byref(o) for o in out])
        return tuple(o.value for o in out)

    # ------------------------------------------------------------------
    def bind(self):
        """hand the members' state and trace pointers and their parameters to the batch (after every member's ``reset``)"""
        n = len(self.members)
        states = (State * n)(*[m.state for m in self.members])
        traces = (C.c_void_p * n)(*[None if m.trace is None else m.trace.data_ptr() for m in self.members])
        self._call("gcsadmm_batch_bind", states, traces, self._stream())

    def reset(self, params=None, **common):
        """``DeviceSolver.reset`` on every member, then ``bind``.  ``common``: parameters of all members; ``params``: a list of one dict per
        member that overrides them (rho, tau_incr, cold_start, ...: every field may differ between members)."""
        per = params if params is not None else [{}] * len(self.members)
        if len(per) != len(self.members):
            raise ValueError("one parameter dict per member")
        for m, p in zip(self.members, per):
            m.reset(**{**common, **p})
        self.bind()

    def enqueue(self, k: int):
        """up to k iterations of every member that is still running, back to back, no host synchronisation"""
        self._call("gcsadmm_batch_run", int(k), self._stream())

    def poll(self):
        """(status, it) of every member, two lists, in one device-to-host copy (synchronises the stream)"""
        n = len(self.members)
        status, it = (C.c_int32 * n)(), (C.c_int32 * n)()
        self._call("gcsadmm_batch_poll", status, it, self._stream())
        return list(status), list(it)

    # ------------------------------------------------------------------ replanning (gcs_admm_amd/transfer.py)
    def _id_table(self, vertex_ids, active):
        """(the checked id arrays, the host array of their addresses) for the members ``active`` says take part"""
        from .transfer import check_vertex_ids
        if vertex_ids is None or len(vertex_ids) != len(self.members):
            raise ValueError("one vertex id list per member")
        ids = [check_vertex_ids(v, m.g.num_vertices) if a else None for v, m, a in zip(vertex_ids, self.members, active)]
        return ids, (C.c_void_p * len(ids))(*[None if a is None else a.ctypes.data for a in ids])

    def export_state(self, vertex_ids):
        """One ``StateSnapshot`` per member of the state it holds now -- typically after ``solve`` --, keyed by ``vertex_ids[i]`` (int32,
        >= 0, strictly ascending with the vertex index of member i): one launch for the whole batch (gcsadmm_batch_export_state).  The
        batch must be bound (``reset`` or ``solve`` has run)."""
        from .transfer import StateSnapshot
        state_dtype = "f64" if not self.members or self.members[0].dtype_code == abi.F64 else "f32"
        ids, table = self._id_table(vertex_ids, [True] * len(self.members))
        snaps = [StateSnapshot(m.g.n, state_dtype, m.g.num_vertices, m.g.num_edges, self.device) for m in self.members]
        self._call("gcsadmm_batch_export_state", table, (C.c_void_p * len(snaps))(*[C.addressof(s.c) for s in snaps]), self._stream())
        return snaps

    def import_state(self, seed, vertex_ids):
        """Write ``seed[i]`` (a ``StateSnapshot`` or None: member i keeps its state) into the state of member i, matched by
        ``vertex_ids[i]``; what the snapshot does not have becomes zero: one launch (gcsadmm_batch_import_state), after ``reset``."""
        if len(seed) != len(self.members):
            raise ValueError("one snapshot or None per member")
        ids, table = self._id_table(vertex_ids, [s is not None for s in seed])
        self._call("gcsadmm_batch_import_state", table, (C.c_void_p * len(seed))(*[None if s is None else C.addressof(s.c) for s in seed]), self._stream())

    def solve(self, chunk: int = 25, params=None, seed=None, vertex_ids=None, **common):
        """Every member to its stop test (or its max_it) as ``DeviceSolver.solve`` runs one: enqueue ``chunk`` iterations, poll once, stop
        when no member is running.  Returns one result per member in the shape ``DeviceSolver.solve`` returns; ``wall_time_s`` is the
        wall time of the whole batch.  ``seed``: one ``StateSnapshot`` or None per member, with ``vertex_ids`` (as ``export_state``):
        after the reset the seeded members start from their snapshot (``import_state``) at the rho their parameters say, the others
        from zero as always; the import is part of ``wall_time_s``."""
        if seed is not None and len(seed) != len(self.members):
            raise ValueError("one snapshot or None per member")
        self.reset(params, **common)
        if seed is not None and any(s is not None for s in seed):
            self.torch.cuda.synchronize(self.device)
            t_import = time.perf_counter()
            self.import_state(seed, vertex_ids)
            t_import = time.perf_counter() - t_import
        else:
            t_import = 0.0
        max_it, done = max(m.params.max_it for m in self.members), 0
        self.torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        while True:
            k = min(chunk, max_it - done)
            if k > 0:
                self.enqueue(k)
                done += k
            status, _ = self.poll()
            if all(s != RUNNING for s in status) or done >= max_it:
                break
        wall = time.perf_counter() - t0 + t_import
        return [m.record(m.read_control(), wall) for m in self.members]
