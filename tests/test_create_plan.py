"""What gcsadmm_create decides, checked without a GPU: gcs_admm_amd/csrc/create_plan.h compiled for the host
(tests/hostemu/plan_emu.cpp, with the workgroup program's LDS sizing built at 256 and at 512 threads, tests/hostemu/wg_sizes.cpp).
The descriptor is the one solver.DeviceSolver hands to gcsadmm_create.  Pinned here: the program of every vertex and its automatic
rules, the wavefront packing, the schedule knobs of include/gcsadmm.h, the region-terminal layout, and the refusals with their
messages.  What the GPU runs with these plans is checked by test_gpu_parity.py / test_gpu_configs.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import BENCHMARKS, star_case
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import convert_pt_to_polytope, graph_from_sets, lattice_boxes
from gcs_admm_amd.abi import graph_desc
from hostemu_lib import emu_path
from test_gpu_configs import _region_row, _region_star

OK, BAD_ARG, UNSUPPORTED = 0, 1, 2          # gcsadmm_status
KB = 1024


def build_lib(out=None, flags=()):
    """the plan shim of hostemu_lib.py; ``out`` and ``flags`` are for builds beside it (tools/sanitize_cpu.sh)"""
    return emu_path("planemu", out, flags)


def load(path):
    lib = C.CDLL(path)
    lib.plan_emu_error.restype = C.c_char_p
    lib.plan_emu_get.restype = C.c_double
    lib.plan_emu_vec.restype = C.c_longlong
    lib.plan_emu_term_ws_doubles.restype = lib.plan_emu_term_record_doubles.restype = lib.plan_emu_warm_record_doubles.restype = C.c_longlong
    return lib


@pytest.fixture(scope="module")
def lib():
    return load(build_lib())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def descriptor(g, columns="incidence", dtype=0, **knobs):
    """(GraphDesc, arrays it points into): what DeviceSolver.__init__ builds (abi.graph_desc); knobs: vertex_program, wave_slots,
    wave_align, wave_store_dl, wave_generic_rows, or any other field to override"""
    d, keep, _ = graph_desc(g, state_dtype=dtype, device=0, columns=columns, num_incidences=2 * g.num_edges if columns == "edge" else None)
    for k, v in knobs.items():
        setattr(d, k, v)
    return d, keep


SCALARS = ["n_term", "term_vtx0", "term_vtx1", "term_is_src0", "term_is_src1", "term_ws_off0", "term_ws_off1", "term_rec_off0",
           "term_rec_off1", "term_ws_doubles", "term_rec_doubles", "term_threads", "term_lds_doubles", "wg_lds_bytes", "wg_box", "wg_t512",
           "n_waves", "slots_cap", "align_rows", "store_dl", "all_m4", "wave_mm", "lds_bytes", "wave_reorder", "wg_reorder",
           "prox_lds_bytes", "nx", "nmu", "edge_unroll", "edge_blocks"]
VECTORS = ["deg_in", "bc", "special_vtx", "special_kind", "wg_vtx", "wave_slot_ptr", "wave_vtx", "warm_ptr", "prox_vtx", "col_owned",
           "col_vertex"]
INT_VECTORS = set(VECTORS) - {"bc"}


class Plan(dict):
    __getattr__ = dict.__getitem__


def make(lib, g, **kw):
    """(status, message, Plan or None)"""
    d, keep = descriptor(g, **kw)
    st = lib.plan_emu_make(C.byref(d))
    if st != OK:
        return st, lib.plan_emu_error().decode(), None
    p = Plan()
    for name in SCALARS:
        v = lib.plan_emu_get(name.encode())
        p[name] = v if name in ("nx", "nmu") else int(v)
    for name in VECTORS:
        size = lib.plan_emu_vec(name.encode(), None, 0)
        buf = np.zeros(size)
        lib.plan_emu_vec(name.encode(), _p(buf), size)
        p[name] = buf.astype(np.int64) if name in INT_VECTORS else buf
    return st, "", p


def plan(lib, g, **kw):
    st, msg, p = make(lib, g, **kw)
    assert st == OK, msg
    return p


def refusal(lib, g, **kw):
    st, msg, _ = make(lib, g, **kw)
    assert st != OK
    return st, msg


def degrees(g):
    deg = np.diff(g.inc_ptr).astype(np.int64)
    din = np.array([int((g.inc_out[g.inc_ptr[v]:g.inc_ptr[v + 1]] == 0).sum()) for v in range(g.num_vertices)])
    return deg, din, np.diff(g.poly_ptr).astype(np.int64)


def generic(g):
    deg, din, _ = degrees(g)
    return [v for v in range(g.num_vertices) if v not in (g.src, g.dst) and din[v] > 0 and deg[v] > din[v]]


def waves(p):
    return [list(p.wave_vtx[p.wave_slot_ptr[w]:p.wave_slot_ptr[w + 1]]) for w in range(p.n_waves)]


def check_common(lib, g, p, t512):
    """what every plan satisfies: a program for every vertex, sizes from the sizing functions, state columns"""
    deg, din, m = degrees(g)
    gen = generic(g)
    region = [p.term_vtx0, p.term_vtx1][:p.n_term]
    assert sorted(list(p.wg_vtx) + list(p.wave_vtx)) == gen
    assert sorted(list(p.special_vtx) + region + gen) == list(range(g.num_vertices))
    kind = dict(zip(p.special_vtx, p.special_kind))
    assert all(kind[v] == (1 if v == g.src else 2 if v == g.dst else 0) for v in kind)
    assert np.array_equal(p.deg_in, din)
    # heaviest workgroup-program sub-problems first; LDS of the heaviest layout at the thread count chosen
    cost = (deg[p.wg_vtx] + 1) * m[p.wg_vtx]
    assert np.all(np.diff(cost) <= 0)
    assert p.wg_t512 == t512
    want = max([lib.plan_emu_wg_lds_bytes(t512, g.n, int(deg[v] + 1), int(m[v]), p.wg_box) for v in p.wg_vtx], default=0)
    assert p.wg_lds_bytes == want
    # wavefronts: groups of d + 1 lanes within 64, at most slots_cap vertices each, vertex order kept
    assert list(p.wave_vtx) == sorted(p.wave_vtx)
    for w in waves(p):
        assert 1 <= len(w) <= p.slots_cap and sum(deg[v] + 1 for v in w) <= 64
    assert p.slots_cap == max([len(w) for w in waves(p)], default=1)
    assert (p.lds_bytes > 0) == (p.n_waves > 0)
    # warm-start records: one per generic vertex
    rec = [lib.plan_emu_warm_record_doubles(g.n, int(m[v]), int(deg[v])) if v in gen else 0 for v in range(g.num_vertices)]
    assert np.array_equal(p.warm_ptr, np.concatenate([[0], np.cumsum(rec)]))
    assert p.wave_reorder == (p.n_waves >= 512) and p.wg_reorder == (len(p.wg_vtx) >= 512)
    assert list(p.prox_vtx) == [v for v in range(g.num_vertices) if v not in (g.src, g.dst)]
    assert p.prox_lds_bytes == lib.plan_emu_wg_lds_bytes(0, g.n, 1, int(m.max(initial=1)), 0)
    owner = np.repeat(np.arange(g.num_vertices), deg)
    assert np.array_equal(p.col_vertex, owner) and np.array_equal(p.col_owned, np.ones_like(owner))
    bc = g.poly_b - np.einsum("jk,jk->j", g.poly_A, g.interior[np.repeat(np.arange(g.num_vertices), m)])
    assert np.allclose(p.bc, bc, rtol=0, atol=1e-12)
    assert p.nx == (4 * g.n + 1) * (g.num_vertices + 2 * g.num_edges) and p.nmu == (4 * g.n + 2) * g.num_edges


@pytest.fixture(scope="module")
def lattice10k():
    return lattice_boxes(100, 100, seed=0)


@pytest.mark.parametrize("name", BENCHMARKS)
def test_benchmarks_run_the_512_thread_workgroup_program(lib, name):
    """the reference's cases: every generic vertex on a 512-thread workgroup (at most 255 of them: one CU each), no wavefronts,
    the terminals points (closed form)"""
    g = load_fixture(name)[1]
    p = plan(lib, g)
    check_common(lib, g, p, t512=1)
    assert p.n_waves == 0 and p.lds_bytes == 0 and sorted(p.wg_vtx) == generic(g)
    assert p.n_term == 0 and {g.src: 1, g.dst: 2}.items() <= dict(zip(p.special_vtx, p.special_kind)).items()
    assert p.wg_box == 0 and not p.wg_reorder


def test_lattice_10k_runs_the_aligned_box_wavefront_program(lib, lattice10k):
    """n = 2 above 1 024 generic vertices: the wavefront program, its box instantiation, row-aligned groups (<= 2 048 wavefronts),
    7 vertices per wavefront; the dual directions stay in LDS while a wavefront needs at most 40 KB"""
    g = lattice10k
    p = plan(lib, g)
    check_common(lib, g, p, t512=0)
    assert len(p.wg_vtx) == 0 and p.n_waves > 0 and p.all_m4 == 2 and p.wave_mm == 4
    assert p.align_rows == 1 and p.n_waves <= 2048 and p.slots_cap == 7 and p.wave_reorder
    with_dl, without = plan(lib, g, wave_store_dl=1), plan(lib, g, wave_store_dl=2)
    assert with_dl.store_dl == 1 and without.store_dl == 0 and with_dl.lds_bytes > without.lds_bytes
    assert p.store_dl == int(with_dl.lds_bytes <= 40 * KB)
    assert p.lds_bytes == (with_dl if p.store_dl else without).lds_bytes
    assert p.edge_blocks == min(2048, -(-g.num_edges // (256 * p.edge_unroll)))


def test_more_than_2048_wavefronts_pack_dense(lib, lattice10k):
    g = lattice10k
    p = plan(lib, g, wave_slots=2)
    check_common(lib, g, p, t512=0)
    assert p.n_waves > 2048 and p.align_rows == 0 and p.slots_cap == 2
    forced = plan(lib, g, wave_slots=2, wave_align=1)
    assert forced.align_rows == 1 and forced.n_waves > 2048


def test_vertex_program_knob(lib, lattice10k):
    """0: automatic (workgroup program up to 1 024 generic vertices at n = 2), 1: wavefront, 2: workgroup, 3: workgroup at 256 threads"""
    small = lattice_boxes(14, 11, seed=7)
    auto, wave, wg, wg256 = (plan(lib, small, vertex_program=k) for k in range(4))
    assert len(auto.wg_vtx) == len(generic(small)) and auto.n_waves == 0 and auto.wg_t512 == 1
    assert len(wave.wg_vtx) == 0 and len(wave.wave_vtx) == len(generic(small)) and wave.all_m4 == 2
    assert wg.wg_t512 == 1 and np.array_equal(wg.wg_vtx, auto.wg_vtx)
    check_common(lib, small, wg256, t512=0)
    assert np.array_equal(wg256.wg_vtx, auto.wg_vtx) and wg256.wg_lds_bytes < wg.wg_lds_bytes      # (the 512-thread reduction area)
    big = plan(lib, lattice10k, vertex_program=2)
    check_common(lib, lattice10k, big, t512=0)
    assert big.n_waves == 0 and big.wg_reorder
    # one more generic vertex than the automatic limit: wavefronts
    g = lattice_boxes(33, 32, seed=1)
    assert len(generic(g)) > 1024 and plan(lib, g).n_waves > 0 and len(plan(lib, g).wg_vtx) == 0
    assert refusal(lib, small, vertex_program=4) == (BAD_ARG, "vertex_program must be 0, 1, 2 or 3")


def test_wave_knobs(lib, lattice10k):
    g = lattice10k
    p = plan(lib, g, wave_slots=3)
    assert p.slots_cap == 3 and max(len(w) for w in waves(p)) == 3
    assert plan(lib, g, wave_align=1).align_rows == 1 and plan(lib, g, wave_align=2).align_rows == 0
    dense = plan(lib, g, wave_align=2)
    assert dense.n_waves <= plan(lib, g).n_waves
    for rows in (1, 2):
        q = plan(lib, g, wave_generic_rows=rows)
        check_common(lib, g, q, t512=0)
        assert q.all_m4 == 0 and np.array_equal(q.wave_vtx, p.wave_vtx)
    # the generic instantiation keeps both kinds of row duals in LDS: more per wavefront than the box one
    assert plan(lib, g, wave_generic_rows=1, wave_store_dl=2).lds_bytes > plan(lib, g, wave_store_dl=2).lds_bytes
    # a polytope that is not a canonical box turns the box instantiation off
    g2 = lattice_boxes(14, 11, seed=7)
    A = g2.poly_A.copy(); v = generic(g2)[0]
    j = g2.poly_ptr[v]
    A[[j, j + 1]] = A[[j + 1, j]]; b = g2.poly_b.copy(); b[[j, j + 1]] = b[[j + 1, j]]      # the same box, facets in another order
    g2.poly_A, g2.poly_b = A, b
    q = plan(lib, g2, vertex_program=1)
    assert q.all_m4 == 0 and q.wave_mm == 4


@pytest.mark.parametrize("n", [3, 6])
def test_box_lattices_use_the_box_workgroup_instantiation(lib, n):
    g = lattice_boxes(6, 5, n=n, seed=1)
    p = plan(lib, g)
    check_common(lib, g, p, t512=1)
    assert p.wg_box == 1 and p.n_waves == 0
    generic_rows = plan(lib, g, wave_generic_rows=1)
    check_common(lib, g, generic_rows, t512=1)
    assert generic_rows.wg_box == 0 and generic_rows.wg_lds_bytes > p.wg_lds_bytes
    # one polytope that is not a canonical box: the generic instantiation for every vertex
    v = generic(g)[0]
    j = g.poly_ptr[v]
    g.poly_A = g.poly_A.copy(); g.poly_A[j] = g.poly_A[j] * 2.0; g.poly_b = g.poly_b.copy(); g.poly_b[j] *= 2.0
    q = plan(lib, g)
    check_common(lib, g, q, t512=1)
    assert q.wg_box == 0 and q.wg_lds_bytes == generic_rows.wg_lds_bytes


def test_degree_above_63_goes_to_the_workgroup_program(lib):
    """n = 2, wavefront program requested: the hub of a star with 2 x 40 incident edges cannot take a wavefront (d + 1 > 64 lanes)"""
    g = graph_from_sets(*star_case(40))
    deg = np.diff(g.inc_ptr)
    p = plan(lib, g, vertex_program=1)
    check_common(lib, g, p, t512=1)
    assert list(p.wg_vtx) == [v for v in generic(g) if deg[v] > 63] and len(p.wg_vtx) == 1
    assert len(p.wave_vtx) == len(generic(g)) - 1


@pytest.mark.parametrize("case", ["row", "star3", "star6"])
def test_region_terminals(lib, case):
    """workspace and record offsets from the terminal kernel's sizing; work arrays in LDS while they fit 48 KB; one wavefront while
    no phase has more than 256 rows (live edges x 2 x facets)"""
    g = {"row": _region_row, "star3": lambda: _region_star(3, 8, seed=3), "star6": lambda: _region_star(6, 30, seed=6)}[case]()
    p = plan(lib, g)
    check_common(lib, g, p, t512=1)
    deg, din, m = degrees(g)
    term = [(p.term_vtx0, p.term_is_src0), (p.term_vtx1, p.term_is_src1)][:p.n_term]
    assert [v for v, _ in term] == [v for v in (g.src, g.dst) if v not in p.special_vtx]
    live = [int(deg[v] - din[v] if s else din[v]) for v, s in term]
    ws = [lib.plan_emu_term_ws_doubles(g.n, int(m[v]), l) for (v, _), l in zip(term, live)]
    rec = [lib.plan_emu_term_record_doubles(g.n, int(m[v]), l) for (v, _), l in zip(term, live)]
    assert [p.term_ws_off0, p.term_ws_off1][:p.n_term] == list(np.cumsum([0] + ws[:-1]))
    assert [p.term_rec_off0, p.term_rec_off1][:p.n_term] == list(np.cumsum([0] + rec[:-1]))
    assert p.term_ws_doubles == sum(ws) and p.term_rec_doubles == sum(rec)
    assert p.term_lds_doubles == (max(ws) if 8 * max(ws) <= 48 * KB else 0)
    rows = max(l * 2 * int(m[v]) for (v, _), l in zip(term, live))
    assert p.term_threads == (64 if rows <= 256 else 256)
    assert {"row": 2, "star3": 1, "star6": 1}[case] == p.n_term
    if case == "star6":
        assert p.term_lds_doubles == 0 and p.term_threads == 256
    if case == "row":
        assert p.term_threads == 64 and p.term_lds_doubles > 0


def _two_boxes():
    A = np.vstack([np.eye(2), -np.eye(2)])
    As, bs = {}, {}
    As['s'], bs['s'] = convert_pt_to_polytope(np.array([0.0, 0.0]))
    As['t'], bs['t'] = convert_pt_to_polytope(np.array([1.5, 0.0]))
    As[0], bs[0] = A, np.array([1.0, 1.0, 1.0, 1.0])
    As[1], bs[1] = A, np.array([2.0, 1.0, -0.5, 1.0])
    return graph_from_sets(As, bs, 2)


def test_refusals(lib):
    """each refusal with the message callers match on, in the order create checks them"""
    g = _two_boxes()
    assert refusal(lib, g, n=9) == (UNSUPPORTED, "the vertex kernels are instantiated for n = 1 .. 8")
    assert refusal(lib, g, num_incidences=int(g.inc_ptr[-1]) - 1) == (BAD_ARG, "inconsistent incidence CSR")
    # incoming after outgoing
    h = _two_boxes()
    v = generic(h)[0]
    lo, hi = h.inc_ptr[v], h.inc_ptr[v + 1]
    h.inc_out = h.inc_out.copy(); h.inc_out[lo:hi] = h.inc_out[lo:hi][::-1]
    assert refusal(lib, h) == (BAD_ARG, "incoming incidences must precede outgoing ones")
    # fewer than n + 1 facets
    h = _two_boxes()
    h.poly_ptr = h.poly_ptr.copy(); h.poly_ptr[v + 1:] -= 2
    assert refusal(lib, h) == (BAD_ARG, "polytope with fewer than n+1 facets cannot be bounded")
    # bad edge-major slots, slot out of range
    d, keep = descriptor(g, columns="edge")
    keep[3][[0, 1]] = keep[3][[1, 0]]
    assert lib.plan_emu_make(C.byref(d)) == BAD_ARG
    assert lib.plan_emu_error().decode() == "edge-major columns: edge_inc_tail[e] must be e and edge_inc_head[e] num_edges + e"
    assert refusal(lib, g, columns="edge", num_incidences=2 * g.num_edges + 1)[1] == "edge-major columns: num_incidences must be 2 num_edges"
    assert refusal(lib, g, edge_major_columns=2)[1] == "edge_major_columns must be 0 or 1"
    h = _two_boxes()
    h.edge_inc_head = h.edge_inc_head.copy(); h.edge_inc_head[0] = h.inc_ptr[-1]
    assert refusal(lib, h)[1] == "edge incidence slot out of range"
    # centre not inside (the terminals are exempt)
    h = _two_boxes()
    h.interior = h.interior.copy(); h.interior[v] = [5.0, 0.0]
    assert refusal(lib, h) == (BAD_ARG, "center is not strictly inside its polytope")
    # the same region as source and target
    h = _region_row()
    assert refusal(lib, h, dst=h.src) == (UNSUPPORTED, "source and target are the same region")
    # a region terminal with nothing on its live side
    A = np.vstack([np.eye(2), -np.eye(2)])
    As, bs = {}, {}
    As['s'], bs['s'] = A, np.array([0.5, 0.5, 0.5, 0.5])
    As['t'], bs['t'] = convert_pt_to_polytope(np.array([3.0, 0.0]))
    As[0], bs[0] = A, np.array([4.0, 1.0, 1.0, 1.0])
    h = graph_from_sets(As, bs, 2, edges=[(0, 's'), (0, 't')])
    st, msg = refusal(lib, h)
    assert st == UNSUPPORTED and "live side" in msg
    # more than 160 KB of LDS: the hub of a star with 2 x 60 incident edges on one workgroup
    assert refusal(lib, graph_from_sets(*star_case(60))) == (UNSUPPORTED, "a vertex sub-problem (degree x facets) does not fit the 160 KB of LDS of a CU")
    # a closed-form vertex above 256 incident edges: the hub of a 2 x 140 star with every edge turned inwards (no flow)
    h = graph_from_sets(*star_case(140))
    hub = int(np.argmax(np.diff(h.inc_ptr)))
    h.inc_out = h.inc_out.copy(); h.inc_out[h.inc_ptr[hub]:h.inc_ptr[hub + 1]] = 0
    assert refusal(lib, h) == (UNSUPPORTED, "terminal vertex degree above 256")
