"""The C ABI of include/gcsadmm.h as Python sees it, in one place: the ctypes mirrors of its structs, its status and dtype codes,
the prototype of every function it declares, and the loader that puts those prototypes on the library (built from gcs_admm_amd/csrc
by ``build.py``).  Importing this module needs neither a GPU nor the library.  tests/test_abi.py holds the table to the header.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgcsadmm.so")

F64, F32 = 0, 1
RUNNING, CONVERGED, MAX_IT, DIVERGED = -1, 0, 1, 2
BATCH_LARGE = 1        # GCSADMM_BATCH_LARGE (gcsadmm_batch_create_ex)
BATCH_TERMINALS = 4    # GCSADMM_BATCH_TERMINALS (bit 1 stays undefined)
STATUS_NAME = {RUNNING: "running", CONVERGED: "converged", MAX_IT: "max_it", DIVERGED: "diverged"}


class GraphDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("num_vertices", C.c_int32), ("num_edges", C.c_int32), ("num_incidences", C.c_int32),
                ("inc_ptr", C.c_void_p), ("inc_edge", C.c_void_p), ("inc_out", C.c_void_p),
                ("edge_inc_tail", C.c_void_p), ("edge_inc_head", C.c_void_p),
                ("poly_ptr", C.c_void_p), ("poly_A", C.c_void_p), ("poly_b", C.c_void_p), ("center", C.c_void_p),
                ("src", C.c_int32), ("dst", C.c_int32), ("state_dtype", C.c_int32), ("device", C.c_int32),
                ("inc_counted", C.c_void_p), ("edge_counted", C.c_void_p),
                ("nx_global", C.c_double), ("nmu_global", C.c_double),
                # schedule of the vertex step (0 = automatic): see include/gcsadmm.h
                ("vertex_program", C.c_int32), ("wave_slots", C.c_int32), ("wave_align", C.c_int32),
                ("wave_store_dl", C.c_int32), ("wave_generic_rows", C.c_int32), ("edge_major_columns", C.c_int32),
                # vertex sub-problems larger than LDS: 0 refused, 1 split form where needed, 2 split form everywhere
                ("vertex_workspace", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("rho", C.c_double), ("tau_incr", C.c_double), ("tau_decr", C.c_double), ("nu", C.c_double),
                ("it_rho_limit", C.c_int32), ("max_it", C.c_int32), ("eps_abs", C.c_double), ("eps_rel", C.c_double),
                ("eps_edge", C.c_double), ("ipm_tol", C.c_double), ("ipm_max_iter", C.c_int32), ("cold_start", C.c_int32)]


class State(C.Structure):
    _fields_ = [("copy", C.c_void_p), ("mu", C.c_void_p), ("zedge", C.c_void_p),
                ("xv", C.c_void_p), ("zv", C.c_void_p), ("yv", C.c_void_p)]


class HaloDesc(C.Structure):
    _fields_ = [("num_peers", C.c_int32), ("peer_rank", C.c_void_p), ("send_ptr", C.c_void_p), ("send_cols", C.c_void_p),
                ("recv_ptr", C.c_void_p), ("recv_cols", C.c_void_p)]


class ControlBlock(C.Structure):
    _fields_ = [("rho", C.c_double), ("mu_scale", C.c_double), ("sums", C.c_double * 5),
                ("pri", C.c_double), ("dual", C.c_double), ("eps_pri", C.c_double), ("eps_dual", C.c_double),
                ("it", C.c_int32), ("status", C.c_int32), ("inner_failures", C.c_int32), ("inner_iters", C.c_int32)]


class Snapshot(C.Structure):
    """gcsadmm_snapshot: device pointers the caller allocates (gcs_admm_amd/transfer.py)"""
    _fields_ = [("n", C.c_int32), ("state_dtype", C.c_int32), ("V", C.c_int32), ("E", C.c_int32),
                ("edge_key", C.c_void_p), ("edge_words", C.c_void_p), ("vertex_id", C.c_void_p), ("vertex_words", C.c_void_p),
                ("rho", C.c_void_p)]


_p, _i, _d = C.c_void_p, C.c_int32, C.c_double
_run, _run_timed = [_p, _p, _i, _p, _p], [_p, _p, _i, _p, _p] + [_p] * 4
_csr = [_i, _i, _p, _p, _p]
# every function of include/gcsadmm.h, in its order: (argument types, result type).  Pointers and handles are c_void_p, so an array
# or a tensor goes in as a plain address (``a.ctypes.data``, ``t.data_ptr()``) and keeps all 64 bits.
PROTOTYPES = {
    "gcsadmm_create": ([_p, _p], _i),
    "gcsadmm_destroy": ([_p], None),
    "gcsadmm_last_error": ([_p], C.c_char_p),
    "gcsadmm_reset": ([_p] * 3, _i),
    "gcsadmm_vertex_step": ([_p] * 3, _i),
    "gcsadmm_edge_step": ([_p] * 4, _i),
    "gcsadmm_control": ([_p] * 4, _i),
    "gcsadmm_run": (_run, _i),
    "gcsadmm_set_fused_tail": ([_p, _i], _i),
    "gcsadmm_read_control": ([_p] * 3, _i),
    "gcsadmm_cost": ([_p, _p, _d, _p, _p], _i),
    "gcsadmm_query": ([_p] * 6, _i),
    "gcsadmm_query_workspace": ([_p] * 4, _i),
    "gcsadmm_unit_iterations": ([_p, _p, _i, _p, _p], _i),
    "gcsadmm_run_timed": (_run_timed, _i),
    # batches of handles (gcs_admm_amd/batch.py)
    "gcsadmm_batch_create": ([_p, _i, _p], _i),
    "gcsadmm_batch_create_ex": ([_p, _i, _i, _p], _i),
    "gcsadmm_batch_query": ([_p] * 4, _i),
    "gcsadmm_batch_query_terminals": ([_p] * 3, _i),
    "gcsadmm_batch_destroy": ([_p], None),
    "gcsadmm_batch_last_error": ([_p], C.c_char_p),
    "gcsadmm_batch_bind": ([_p] * 4, _i),
    "gcsadmm_batch_run": ([_p, _i, _p], _i),
    "gcsadmm_batch_poll": ([_p] * 4, _i),
    # replanning: the state of a solved handle carried to another query graph (gcs_admm_amd/transfer.py)
    "gcsadmm_export_state": ([_p] * 5, _i),
    "gcsadmm_import_state": ([_p] * 5, _i),
    "gcsadmm_batch_export_state": ([_p] * 4, _i),
    "gcsadmm_batch_import_state": ([_p] * 4, _i),
    "gcsadmm_vertex_prox": ([_p] * 6 + [_d, _i, _p, _p], _i),
    # vertex partitions across GPUs (RCCL)
    "gcsadmm_comm_unique_id": ([_p], _i),
    "gcsadmm_attach_comm": ([_p, _i, _i, _p, _p], _i),
    "gcsadmm_check_halo": ([_p, _i, _i, _p], _i),
    "gcsadmm_run_partitioned": (_run, _i),
    "gcsadmm_run_partitioned_timed": (_run_timed, _i),
    "gcsadmm_set_overlap": ([_p, _i, _p], _i),
    "gcsadmm_comm_count": ([_p, _p], _i),
    "gcsadmm_halo_pack": ([_p] * 3, _i),
    "gcsadmm_halo_unpack": ([_p] * 3, _i),
    "gcsadmm_halo_exchange": ([_p] * 3, _i),
    "gcsadmm_halo_buffers": ([_p] * 4, _i),
    # graph construction at scale (gcs_admm_amd/scene.py): batch calls, then the same pipeline on a resident scene
    "gcsadmm_polytope_last_error": ([], C.c_char_p),
    "gcsadmm_polytope_centers": (_csr + [_i, _p, _p, _p], _i),
    "gcsadmm_polytope_bounds": (_csr + [_p, _i, _p, _p, _p], _i),
    "gcsadmm_polytope_overlaps": (_csr + [_p, C.c_long, _p, _p, _d, _i, _p, _p], _i),
    "gcsadmm_scene_create": (_csr + [_i, _p], _i),
    "gcsadmm_scene_destroy": ([_p], None),
    "gcsadmm_scene_centers": ([_p] * 4, _i),
    "gcsadmm_scene_bounds": ([_p] * 4, _i),
    "gcsadmm_scene_set_boxes": ([_p] * 3, _i),
    "gcsadmm_scene_candidate_pairs": ([_p, _d, _p], _i),
    "gcsadmm_scene_overlaps": ([_p, _d, _p, _p], _i),
    "gcsadmm_scene_read_pairs": ([_p] * 5, _i),
    # the rounding step's path restrictions on a resident scene (gcs_admm_amd/rounding.py)
    "gcsadmm_scene_restrict_paths": ([_p, _i, _p, _p, _p, _d, _i, _p, _p, _p, _p], _i),
    # the regions under query points on a resident scene (gcs_admm_amd/queries.py)
    "gcsadmm_scene_locate_points": ([_p, _i, _p, _d, _d, _p], _i),
    "gcsadmm_scene_locate_boxes": ([_p, _i, _p, _p, _d, _p], _i),
    "gcsadmm_scene_read_hits": ([_p] * 4, _i),
    # ... and the nearest regions of points that may lie in none (csrc/point_project_core.h)
    "gcsadmm_scene_project_points": ([_p, _i, _p, _p, _i, _p], _i),
    "gcsadmm_scene_read_projections": ([_p] * 5, _i),
    # ... and the regions segments run through, with the cover test (csrc/segment_clip_core.h)
    "gcsadmm_scene_clip_segments": ([_p, _i, _p, _p, _d, _p, _p], _i),
    "gcsadmm_scene_read_spans": ([_p] * 3, _i),
    "gcsadmm_scene_read_cover": ([_p] * 5, _i),
    # edits of a decided scene
    "gcsadmm_scene_add_regions": ([_p, _i, _p, _p, _p, _d, _d] + [_p] * 6, _i),
    "gcsadmm_scene_remove_regions": ([_p, _i, _p, _p], _i),
    "gcsadmm_scene_read_regions": ([_p] * 7, _i),
    # the region graph of a decided scene and the query graphs of a batch from it (csrc/query_graph_core.h)
    "gcsadmm_scene_build_region_graph": ([_p] * 3, _i),
    "gcsadmm_scene_read_region_graph": ([_p] * 5, _i),
    "gcsadmm_scene_query_graphs": ([_p, _i, _p, _p, _p, _i] + [_p] * 8, _i),
    # the informed region set of every query of a batch (csrc/informed_core.h)
    "gcsadmm_scene_region_paths": ([_p, _i, _p, _p, _p, _i] + [_p] * 4, _i),
    "gcsadmm_scene_informed_regions": ([_p, _i, _p, _p, _d, _p, _p], _i),
    # ... between start and goal sets (csrc/informed_set_core.h)
    "gcsadmm_scene_region_paths_sets": ([_p, _i, _p, _p, _p, _p, _i] + [_p] * 4, _i),
    "gcsadmm_scene_informed_regions_sets": ([_p, _i, _p, _p, _p, _d, _p, _p], _i),
    # the query graphs of a batch on each query's kept regions (csrc/induced_graph_core.h)
    "gcsadmm_scene_induced_sizes": ([_p, _i] + [_p] * 6, _i),
    "gcsadmm_scene_induced_query_graphs": ([_p, _i, _p, _p, _p, _p, _i] + [_p] * 9, _i),
    # the candidate paths of the rounding step, drawn on the device (gcs_admm_amd/walks.py)
    "gcsadmm_walks_create": ([_i] + [_p] * 7 + [_i, _p], _i),
    "gcsadmm_walks_destroy": ([_p], None),
    "gcsadmm_walks_last_error": ([_p], C.c_char_p),
    "gcsadmm_walks_sample": ([_p, _p, _i, _p, _i, _i, _i] + [_p] * 4, _i),
}
EXPORTS = list(PROTOTYPES)


class GcsAdmmError(RuntimeError):
    pass


def check(status, message):
    """raise GcsAdmmError(message()) unless ``status`` is 0 (or None: a void function)"""
    if status:
        raise GcsAdmmError(message())


_lib = None        # the one library of this process


def select_library(path: str) -> None:
    """Make ``path`` (a build.variant(..) of the library) the one every handle of this process runs.  The only way to change LIB_PATH:
    a process that has already loaded another library is refused, so no run mixes two."""
    global LIB_PATH
    path = os.path.abspath(path)
    if _lib is not None and _lib._name != path:
        raise RuntimeError(f"{_lib._name} is already loaded: select {path} before the first handle is made")
    LIB_PATH = path


def load_library() -> C.CDLL:
    """dlopen the library at LIB_PATH and declare every prototype on it; fail loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -m gcs_admm_amd.build` (hipcc, gfx950). "
                               "There is no CPU fallback.")
        # PyTorch-ROCm ships its own HIP runtime (same SONAME as /opt/rocm's): it must be the one already
        # loaded when libgcsadmm.so resolves libamdhip64, or the process ends up with two runtimes and
        # the tensors' device pointers mean nothing to the library.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (argtypes, restype) in PROTOTYPES.items():
            f = getattr(lib, name)
            f.argtypes, f.restype = argtypes, restype
        _lib = lib
    return _lib


def graph_desc(g, *, state_dtype, device, num_incidences=None, inc_counted=None, edge_counted=None, nx_global=0.0,
               nmu_global=0.0, columns="incidence", **knobs):
    """The descriptor gcsadmm_create takes for graph ``g`` (gcs_admm_amd.graph.GcsGraph), filled by field name.  ``state_dtype``: F64 or
    F32; ``columns``: "incidence" or "edge" (solver.DeviceSolver) -- for "edge" the two slot arrays and ``inc_counted``, which come
    in incidence numbering, are renumbered; ``knobs``: the schedule fields of GraphDesc (vertex_program, wave_*, vertex_workspace).
    Returns (GraphDesc, the arrays it points into -- keep them alive as long as it is used, col_of: incidence column -> state column)."""
    if columns not in ("incidence", "edge"):
        raise ValueError("columns must be 'incidence' or 'edge'")
    E = g.num_edges
    NI = int(num_incidences) if num_incidences is not None else int(g.inc_ptr[-1])
    tail, head = g.edge_inc_tail.astype(np.int32), g.edge_inc_head.astype(np.int32)
    col_of = np.arange(NI, dtype=np.int64)
    if columns == "edge":
        if NI != 2 * E:
            raise ValueError("edge-major columns need exactly two columns per edge")
        col_of = np.empty(NI, dtype=np.int64)
        col_of[tail] = np.arange(E); col_of[head] = E + np.arange(E)
        tail, head = np.arange(E, dtype=np.int32), (E + np.arange(E)).astype(np.int32)
        if inc_counted is not None:
            ic = np.empty(NI, dtype=np.uint8)
            ic[col_of] = np.asarray(inc_counted, dtype=np.uint8)
            inc_counted = ic
    arrays = dict(inc_ptr=g.inc_ptr.astype(np.int32), inc_edge=g.inc_edge.astype(np.int32), inc_out=g.inc_out.astype(np.int32),
                  edge_inc_tail=tail, edge_inc_head=head, poly_ptr=g.poly_ptr.astype(np.int32), poly_A=g.poly_A.astype(np.float64),
                  poly_b=g.poly_b.astype(np.float64), center=g.interior.astype(np.float64),
                  inc_counted=None if inc_counted is None else np.asarray(inc_counted, dtype=np.uint8),
                  edge_counted=None if edge_counted is None else np.asarray(edge_counted, dtype=np.uint8))
    arrays = {k: None if a is None else np.ascontiguousarray(a) for k, a in arrays.items()}
    desc = GraphDesc(n=g.n, num_vertices=g.num_vertices, num_edges=E, num_incidences=NI, src=g.src, dst=g.dst,
                     state_dtype=state_dtype, device=device, nx_global=float(nx_global), nmu_global=float(nmu_global),
                     edge_major_columns=int(columns == "edge"), **{k: int(v) for k, v in knobs.items()},
                     **{k: None if a is None else a.ctypes.data for k, a in arrays.items()})
    return desc, list(arrays.values()), col_of
