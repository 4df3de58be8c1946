"""Host side of the MI355X ADMM loop: the driver that mirrors the reference's main loop (admm_solver_v3.py:621-733) over the C ABI
(include/gcsadmm.h, built from gcs_admm_amd/csrc by ``build.py``; its Python binding is gcs_admm_amd/abi.py).

Device buffers are PyTorch-ROCm tensors; the library only ever sees their
``data_ptr()`` and the current HIP stream.  There is NO fallback: if the HIP
library is missing or no GPU is visible this module raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import time
from typing import Optional

import numpy as np

from . import abi
from .abi import (CONVERGED, DIVERGED, EXPORTS, F32, F64, MAX_IT, RUNNING, STATUS_NAME,  # noqa: F401  (re-exported)
                  ControlBlock, GcsAdmmError, GraphDesc, HaloDesc, Params, State)
from .graph import GcsGraph


load_library = abi.load_library


def halo_arrays(send_idx, recv_idx):
    """The halo lists of a vertex partition (gcs_admm_amd.partition.LocalPartition.send_idx / recv_idx: neighbour rank ->
    columns in canonical (global edge, side) order) as the flat CSR arrays of ``gcsadmm_halo_desc``: peers in ascending
    rank order, send and receive lists of a peer equally long.  Returns (peer_rank, ptr, send_cols, recv_cols) int32."""
    peers = sorted(send_idx)
    if sorted(recv_idx) != peers:
        raise ValueError("a partition sends to and receives from the same neighbours")
    cnt = [len(send_idx[r]) for r in peers]
    if cnt != [len(recv_idx[r]) for r in peers]:
        raise ValueError("send and receive lists of a neighbour must be equally long")
    ptr = np.zeros(len(peers) + 1, np.int32); ptr[1:] = np.cumsum(cnt)
    cat = lambda d: (np.concatenate([np.asarray(d[r], np.int32) for r in peers]) if peers else np.zeros(0, np.int32))
    return np.asarray(peers, np.int32), ptr, np.ascontiguousarray(cat(send_idx)), np.ascontiguousarray(cat(recv_idx))


class DeviceSolver:
    """One GCS instance (or one vertex partition of it) resident on one MI355X.

    ``graph`` is the integer/CSR description (gcs_admm_amd.graph.GcsGraph).  For
    a partition, ``num_incidences`` > ``inc_ptr[-1]`` adds ghost copy slots and
    ``inc_counted`` / ``edge_counted`` implement the ownership rule of the
    global norms.

    ``columns``: numbering of the state columns of ``copy`` / ``mu``.  "incidence" (default): column k = position k of
    the vertex CSR, the numbering ``graph`` and every per-column argument (``inc_counted``, halo lists) are written in.
    "edge": tail side of edge e in column e, head side in column E + e -- the edge step becomes a pure stream (the layout for
    large graphs, include/gcsadmm.h ``edge_major_columns``).  Arguments stay in incidence numbering either way; ``col_of``
    maps an incidence column to the state column, and ``copy[:, col_of]`` is the state in incidence order.

    ``vertex_workspace``: vertices whose sub-problem does not fit a CU's LDS.  0 (default): refused.  1: solved with their edge
    blocks in a device-memory workspace (include/gcsadmm.h ``vertex_workspace``).  2: every workgroup-program vertex that way
    (tests, tuning).  ``query_workspace()`` reports what was placed there.
    """

    def __init__(self, graph: GcsGraph, state_dtype: str = "f64", device: Optional[int] = None,
                 num_incidences: Optional[int] = None, inc_counted=None, edge_counted=None,
                 nx_global: float = 0.0, nmu_global: float = 0.0, program: str = "auto", wave_slots: int = 0,
                 wave_align: int = 0, wave_store_dl: int = 0, wave_generic_rows: int = 0, columns: str = "incidence",
                 vertex_workspace: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: the ADMM loop only runs on the GPU (no CPU fallback)")
        self.torch = torch
        self.lib = load_library()
        self.g = g = graph
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.dtype_code = {"f64": F64, "f32": F32}[state_dtype]
        self.tdtype = torch.float64 if state_dtype == "f64" else torch.float32
        desc, self._keep, self.col_of = abi.graph_desc(
            g, state_dtype=self.dtype_code, device=self.device_index, num_incidences=num_incidences, inc_counted=inc_counted,
            edge_counted=edge_counted, nx_global=nx_global, nmu_global=nmu_global, columns=columns,
            vertex_program={"auto": 0, "wavefront": 1, "workgroup": 2, "workgroup256": 3}[program], wave_slots=wave_slots,
            wave_align=wave_align, wave_store_dl=wave_store_dl, wave_generic_rows=wave_generic_rows, vertex_workspace=vertex_workspace)
        self.NI, self.edge_major = desc.num_incidences, columns == "edge"
        h = C.c_void_p()
        self._call("gcsadmm_create", C.byref(desc), C.byref(h), handle=False, select=False)
        self.h = h
        c, E, V, n = g.c, g.num_edges, g.num_vertices, g.n
        z = lambda *s, dt=self.tdtype: torch.zeros(*s, dtype=dt, device=self.device)
        # (at least one column each: an empty tensor has a null data pointer, which the ABI rejects)
        self.copy, self.mu, self.zedge = z(c, max(self.NI, 1)), z(c, max(self.NI, 1)), z(c, max(E, 1))
        self.xv, self.zv, self.yv = z(V, 2 * n, dt=torch.float64), z(V, 2 * n, dt=torch.float64), z(V, dt=torch.float64)
        self.sums = z(5, dt=torch.float64)
        self._cost = z(1, dt=torch.float64)
        self.state = State(self.copy.data_ptr(), self.mu.data_ptr(), self.zedge.data_ptr(),
                           self.xv.data_ptr(), self.zv.data_ptr(), self.yv.data_ptr())
        self.params = None
        self.trace = None

    # ------------------------------------------------------------------
    def _call(self, name, *args, handle=True, select=True):
        """The one call into the library: ``name(self.h, *args)`` (``handle=False``: ``name(*args)``, and the error text is the calling
        thread's); a status other than 0 raises GcsAdmmError.  ``select``: with the handle's device current -- the stream handed over is
        torch's current stream OF THAT DEVICE, and a null stream handle is bound by HIP to whatever device is current.  The calls made
        without it rely on the library working on the handle's device; a poll of the loop is 2 us shorter (profiles/abi_binding)."""
        h = self.h if handle else None
        with self.torch.cuda.device(self.device) if select else contextlib.nullcontext():
            st = getattr(self.lib, name)(*((h,) if handle else ()), *args)
        abi.check(st, lambda: f"{name} failed ({st}): {self.lib.gcsadmm_last_error(h).decode()}")

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        if getattr(self, "h", None):
            self._call("gcsadmm_destroy", select=False)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------
    def reset(self, rho=1.0, tau_incr=2.0, tau_decr=2.0, nu=10.0, it_rho_limit=100, max_it=1000, eps_abs=1e-4,
              eps_rel=1e-3, eps_edge=1e-4, ipm_tol=None, ipm_max_iter=60, zero_state=True, cold_start=False):
        """Start a loop with the reference's literals as defaults (admm_solver_v3.py:621-651).  ``cold_start``: every vertex
        solve starts from the fixed interior point instead of the record its previous solve left (csrc/warm_start.h)."""
        if ipm_tol is None:
            from . import IPM_TOL as ipm_tol      # the package default (gcs_admm_amd/__init__.py)
        self.params = Params(rho, tau_incr, tau_decr, nu, it_rho_limit, max_it, eps_abs, eps_rel, eps_edge,
                             ipm_tol, ipm_max_iter, 1 if cold_start else 0)
        if zero_state:
            for t in (self.copy, self.mu, self.zedge, self.xv, self.zv, self.yv):
                t.zero_()
        self.trace = self.torch.zeros(max_it, 6, dtype=self.torch.float64, device=self.device)
        self._call("gcsadmm_reset", C.byref(self.params), self._stream())

    def vertex_step(self):
        self._call("gcsadmm_vertex_step", C.byref(self.state), self._stream())

    def edge_step(self):
        self._call("gcsadmm_edge_step", C.byref(self.state), self.sums.data_ptr(), self._stream())
        return self.sums

    def control(self, sums=None):
        s = self.sums if sums is None else sums
        self._call("gcsadmm_control", s.data_ptr(), self.trace.data_ptr(), self._stream())

    def enqueue(self, k: int):
        """k iterations back to back, no host synchronisation."""
        self._call("gcsadmm_run", C.byref(self.state), int(k), self.trace.data_ptr(), self._stream())

    def set_fused_tail(self, mode: int = 1) -> bool:
        """Launches per iteration of ``enqueue`` (include/gcsadmm.h gcsadmm_set_fused_tail): 0 two (vertex step; edge + control step),
        1 automatic -- one on small graphs, where the last vertex workgroup runs the edge and control steps.  Same numbers either
        way.  Returns whether ``enqueue`` fuses on this handle."""
        return bool(self.lib.gcsadmm_set_fused_tail(self.h, int(mode)))

    def enqueue_timed(self, k: int):
        vm, em = C.c_float(0), C.c_float(0)
        vl, el = C.c_int32(0), C.c_int32(0)
        self._call("gcsadmm_run_timed", C.byref(self.state), int(k), self.trace.data_ptr(), self._stream(),
                   C.byref(vm), C.byref(vl), C.byref(em), C.byref(el))
        return dict(vertex_ms=vm.value, vertex_launches=vl.value, edge_ms=em.value, edge_launches=el.value)

    def vertex_prox(self, q, c, ipm_tol: float = 1e-10, ipm_max_iter: int = 60):
        """The x-update of the reference's vertex-edge splits (admm_solver_v1.py:334-383) for every vertex: q, c are
        [V, 4n+1] (weights and centres of the separable quadratic on (x_v, z_v, y_v)).  Returns (xv, zv, yv, failures)."""
        torch = self.torch
        V, n = self.g.num_vertices, self.g.n
        qd = torch.as_tensor(np.ascontiguousarray(q, dtype=np.float64), device=self.device)
        cd = torch.as_tensor(np.ascontiguousarray(c, dtype=np.float64), device=self.device)
        assert qd.shape == (V, 4 * n + 1) and cd.shape == qd.shape
        xv = torch.zeros(V, 2 * n, dtype=torch.float64, device=self.device); zv = torch.zeros_like(xv)
        yv = torch.zeros(V, dtype=torch.float64, device=self.device)
        fails = C.c_int32(0)
        self._call("gcsadmm_vertex_prox", qd.data_ptr(), cd.data_ptr(), xv.data_ptr(), zv.data_ptr(), yv.data_ptr(),
                   float(ipm_tol), int(ipm_max_iter), C.byref(fails), self._stream(), select=False)
        return xv, zv, yv, fails.value

    # ---- vertex partition across GPUs -------------------------------------------------
    def unique_id(self) -> bytes:
        """128 bytes naming a new RCCL communicator (rank 0 creates it, the host distributes it)"""
        buf = (C.c_ubyte * 128)()
        self._call("gcsadmm_comm_unique_id", buf, handle=False, select=False)
        return bytes(buf)

    def _halo_desc(self, send_idx, recv_idx):
        peers, ptr, sc, rc = halo_arrays(send_idx, recv_idx)
        if self.edge_major:      # the lists are written in incidence columns
            sc = np.ascontiguousarray(self.col_of[sc].astype(np.int32)); rc = np.ascontiguousarray(self.col_of[rc].astype(np.int32))
        self._halo_keep = (peers, ptr, sc, rc)
        return HaloDesc(len(peers), peers.ctypes.data, ptr.ctypes.data, sc.ctypes.data, ptr.ctypes.data, rc.ctypes.data)

    def check_halo(self, rank: int, world: int, send_idx, recv_idx):
        """The local checks of ``attach_comm`` alone (no collective): call on every rank and agree on the outcome first."""
        self._call("gcsadmm_check_halo", int(rank), int(world), C.byref(self._halo_desc(send_idx, recv_idx)), select=False)

    def attach_comm(self, rank: int, world: int, unique_id, send_idx, recv_idx):
        """Join the communicator (collective) and upload this partition's halo lists.  ``unique_id`` None: no communicator (the
        host moves the packed halo itself; ``enqueue_partitioned`` then works for world 1 only, without an all-reduce)."""
        idb = (C.c_ubyte * 128).from_buffer_copy(unique_id) if unique_id is not None else None
        self._call("gcsadmm_attach_comm", int(rank), int(world), idb, C.byref(self._halo_desc(send_idx, recv_idx)))
        self.has_comm = unique_id is not None

    def enqueue_partitioned(self, k: int):
        """k iterations of the partitioned loop back to back on the current stream (every rank enqueues the same k)"""
        self._call("gcsadmm_run_partitioned", C.byref(self.state), int(k), self.trace.data_ptr(), self._stream())

    def enqueue_partitioned_timed(self, k: int):
        """k iterations of the partitioned loop with every stage bracketed by HIP events (collective); device ms per stage"""
        v, hl, e, r = (C.c_float(0) for _ in range(4))
        self._call("gcsadmm_run_partitioned_timed", C.byref(self.state), int(k), self.trace.data_ptr(), self._stream(),
                   C.byref(v), C.byref(hl), C.byref(e), C.byref(r))
        return dict(vertex_ms=v.value, halo_ms=hl.value, edge_ms=e.value, reduce_ms=r.value)

    def set_overlap(self, mode: int = 0) -> int:
        """Schedule of the partitioned loop (include/gcsadmm.h gcsadmm_set_overlap): 0 automatic (overlapped when the partition has
        neighbours), 1 overlapped even without neighbours (tests), 2 serial.  Returns the number of boundary wavefronts (0: serial)."""
        n = C.c_int32(0)
        self._call("gcsadmm_set_overlap", int(mode), C.byref(n))
        return n.value

    def comm_count(self) -> int:
        """ranks of the attached RCCL communicator as RCCL reports them (0: none attached)"""
        n = C.c_int32(0)
        self._call("gcsadmm_comm_count", C.byref(n), select=False)
        return n.value

    def halo_pack(self):
        self._call("gcsadmm_halo_pack", C.byref(self.state), self._stream(), select=False)

    def halo_unpack(self):
        self._call("gcsadmm_halo_unpack", C.byref(self.state), self._stream(), select=False)

    def halo_exchange(self):
        self._call("gcsadmm_halo_exchange", C.byref(self.state), self._stream(), select=False)

    def halo_buffers(self):
        """(send pointer, receive pointer, elements) of the packed halo buffers (device memory owned by the handle)"""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        self._call("gcsadmm_halo_buffers", C.byref(a), C.byref(b), C.byref(n), select=False)
        return a.value, b.value, n.value

    def read_control(self) -> ControlBlock:
        cb = ControlBlock()
        self._call("gcsadmm_read_control", C.byref(cb), self._stream(), select=False)
        return cb

    def query(self):
        a, b, c, d, e = (C.c_int32(0) for _ in range(5))
        self._call("gcsadmm_query", C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e), select=False)
        return dict(num_waves=a.value, lds_bytes=b.value, num_special=c.value, num_workgroup_vertices=d.value,
                    workgroup_lds_bytes=e.value)

    def query_workspace(self):
        """the split form of the workgroup program (``vertex_workspace``): its vertices, LDS per workgroup, device workspace bytes"""
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._call("gcsadmm_query_workspace", C.byref(a), C.byref(b), C.byref(c), select=False)
        return dict(num_split_vertices=a.value, split_lds_bytes=b.value, workspace_bytes=c.value)

    def unit_iterations(self):
        """Newton iterations of the last vertex step per dispatch unit (empty for handles with fewer than 512 units)."""
        n = C.c_int32(0)
        self._call("gcsadmm_unit_iterations", None, 0, C.byref(n), self._stream())
        out = np.zeros(n.value, np.int32)
        if n.value:
            self._call("gcsadmm_unit_iterations", out.ctypes.data, n.value, C.byref(n), self._stream())
        return out

    # ---- replanning (gcs_admm_amd/transfer.py) ------------------------------------------
    def export_state(self, vertex_ids):
        """a ``StateSnapshot`` of the state this solver holds, keyed by ``vertex_ids`` (int32, >= 0, strictly ascending with the vertex
        index): gcsadmm_export_state, after ``reset``"""
        from .transfer import StateSnapshot, check_vertex_ids
        ids = check_vertex_ids(vertex_ids, self.g.num_vertices)
        snap = StateSnapshot(self.g.n, "f64" if self.dtype_code == F64 else "f32", self.g.num_vertices, self.g.num_edges, self.device)
        self._call("gcsadmm_export_state", C.byref(self.state), ids.ctypes.data, C.byref(snap.c), self._stream())
        return snap

    def import_state(self, snapshot, vertex_ids):
        """every word of the state from ``snapshot``, matched by ``vertex_ids``; what it does not have becomes zero (gcsadmm_import_state,
        after ``reset(zero_state=...)`` either way: the import writes all six arrays)"""
        from .transfer import check_vertex_ids
        ids = check_vertex_ids(vertex_ids, self.g.num_vertices)
        self._call("gcsadmm_import_state", C.byref(self.state), ids.ctypes.data, C.byref(snapshot.c), self._stream())

    def cost(self) -> float:
        eps = self.params.eps_edge if self.params is not None else 1e-4
        self._call("gcsadmm_cost", C.byref(self.state), eps, self._cost.data_ptr(), self._stream(), select=False)
        return float(self._cost.item())

    # ------------------------------------------------------------------
    def _loop(self, enqueue, chunk, params, clock=False):
        """``reset(**params)``, then ``enqueue(k)`` (which may return device milliseconds to add up) in chunks of ``chunk`` iterations,
        polling the device control block after each, to the stop test or max_it.  ``clock``: the device is idle when the wall clock
        starts.  Returns (control block, wall seconds, device milliseconds)."""
        self.reset(**params)
        max_it, done, dev_ms = self.params.max_it, 0, 0.0
        if clock:
            self.torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        while True:
            k = min(chunk, max_it - done)
            if k > 0:
                dev_ms += enqueue(k) or 0.0
                done += k
            cb = self.read_control()
            if cb.status != RUNNING or done >= max_it:
                return cb, time.perf_counter() - t0, dev_ms

    def solve_partitioned(self, chunk: int = 25, **params):
        """The partitioned loop to its stop test: as ``solve`` but through gcsadmm_run_partitioned (collective)."""
        return self._loop(self.enqueue_partitioned, chunk, params)[0]

    def solve(self, chunk: int = 25, timed: bool = False, **params):
        """Run the loop to its stop test (or max_it), polling the device control
        block every ``chunk`` iterations; returns the reference's record fields
        (utils.py:212-229 naming) plus solver statistics.

        ``timed``: bracket every kernel launch with HIP events (gcsadmm_run_timed) and report ``device_time_s``, the
        summed device time of the vertex-step and edge-step kernels -- the counterpart of the reference's
        ``solve_time``, which adds up SolveInParallel and the edge loop only (admm_solver_v3.py:489-491, 579-585,
        660, 677).  ``wall_time_s`` is the host wall time of the loop either way."""
        def enqueue_timed(k):
            tm = self.enqueue_timed(k)
            return tm["vertex_ms"] + tm["edge_ms"]
        cb, wall, dev_ms = self._loop(enqueue_timed if timed else self.enqueue, chunk, params, clock=True)
        return self.record(cb, wall, dev_ms * 1e-3 if timed else None)

    def record(self, cb, wall_time_s, device_time_s=None):
        """what ``solve`` returns, from the final control block and the trace (batch.BatchSolver builds its members' results with it)"""
        tr = self.trace[:min(cb.it, self.params.max_it)].cpu().numpy()
        return dict(iterations=int(cb.it), status=STATUS_NAME[cb.status],
                    rho_seq=np.concatenate([[self.params.rho], tr[:, 0]]),
                    pri_res_seq=np.concatenate([[0.0], tr[:, 1]]),
                    dual_res_seq=np.concatenate([[0.0], tr[:, 2]]),
                    eps_pri_seq=tr[:, 3], eps_dual_seq=tr[:, 4],
                    inner_failures=int(tr[:, 5].sum()), cost=self.cost(),
                    wall_time_s=wall_time_s, device_time_s=device_time_s)
