"""gcsadmm_graph_desc.vertex_workspace in gcsadmm_create's plan (csrc/create_plan.h), without a GPU: which vertices go to the split form
of the workgroup program (edge blocks in a device-memory workspace), the workspace layout, the refusals.  The shim is plan_emu.cpp with
the split fields added (tests/hostemu/plan_ws_emu.cpp); descriptors and plans are read as in test_create_plan.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import BENCHMARKS, star_case
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import graph_from_sets, lattice_boxes
from hostemu_lib import emu_library
from test_create_plan import BAD_ARG, KB, OK, UNSUPPORTED, descriptor, make, _p
from test_gpu_vertex_workspace import hub_case

OLD_MSG = "a vertex sub-problem (degree x facets) does not fit the 160 KB of LDS of a CU"
POLY_MSG = "a vertex's border system and polytope do not fit the 160 KB of LDS of a CU"


@pytest.fixture(scope="module")
def lib():
    lib = emu_library("planwsemu")
    lib.plan_emu_error.restype = C.c_char_p
    lib.plan_emu_get.restype = C.c_double
    lib.plan_emu_vec.restype = C.c_longlong
    lib.plan_ws_emu_vec.restype = C.c_longlong
    lib.plan_ws_emu_get.restype = C.c_double
    return lib


def full_plan(lib, g, **kw):
    """test_create_plan's Plan plus split_vtx, split_off, split_doubles, split_lds_bytes"""
    st, msg, p = make(lib, g, **kw)
    assert st == OK, msg
    for name in ("split_vtx", "split_off"):
        size = lib.plan_ws_emu_vec(name.encode(), None, 0)
        buf = np.zeros(size)
        lib.plan_ws_emu_vec(name.encode(), _p(buf), size)
        p[name] = buf.astype(np.int64)
    for name in ("split_doubles", "split_lds_bytes"):
        p[name] = int(lib.plan_ws_emu_get(name.encode()))
    return p


def refusal(lib, g, **kw):
    st, msg, _ = make(lib, g, **kw)
    return st, msg


def wg_bytes(lib, t512, n, units, m, box=False):
    return lib.plan_emu_wg_lds_bytes(int(t512), n, units, m, int(box))


def star(k):
    As, bs, n = star_case(k)
    return graph_from_sets(As, bs, n)


def test_mode_0_still_refuses_the_hub(lib):
    g = star(60)
    assert np.diff(g.inc_ptr).max() >= 120
    assert refusal(lib, g) == (UNSUPPORTED, OLD_MSG)
    assert refusal(lib, g, vertex_workspace=0) == (UNSUPPORTED, OLD_MSG)


def test_mode_1_splits_exactly_the_hub(lib):
    g = star(60)
    deg, m = np.diff(g.inc_ptr), np.diff(g.poly_ptr)
    hub = int(np.argmax(deg))
    p = full_plan(lib, g, vertex_workspace=1)
    assert list(p.split_vtx) == [hub] and list(p.split_off) == [0]
    assert hub not in set(p.wg_vtx) and hub not in set(p.wave_vtx)
    # LDS: the layout without units (WL<N>::total(0, m)); slab: what the units add, rounded up to 256 bytes
    box = bool(p.wg_box)
    lds0 = wg_bytes(lib, 0, 2, 0, int(m[hub]), box)
    assert p.split_lds_bytes == lds0 == 8 * lib.plan_ws_emu_split_lds_doubles(2, int(m[hub]), int(box))
    units = wg_bytes(lib, 0, 2, int(deg[hub]) + 1, int(m[hub]), box) - lds0
    assert units > 160 * KB - lds0 and p.split_doubles == -(-units // 256) * 32
    # every other vertex where mode 0 would have put it
    for v in p.wg_vtx:
        assert wg_bytes(lib, p.wg_t512, 2, int(deg[v]) + 1, int(m[v])) <= 160 * KB


def test_slabs_follow_the_layout_heaviest_first(lib):
    """two oversized hubs: offsets are the running sum of the 256-byte rounded slabs, heaviest sub-problem first"""
    from test_gpu_vertex_workspace import mixed_case
    g = mixed_case()
    deg, m = np.diff(g.inc_ptr), np.diff(g.poly_ptr)
    p = full_plan(lib, g, vertex_workspace=2)
    assert len(p.split_vtx) == len(set(p.split_vtx)) >= 2 and len(p.wg_vtx) == 0
    w = (deg[p.split_vtx] + 1) * m[p.split_vtx]
    assert (np.diff(w) <= 0).all()
    off = 0
    for v, o in zip(p.split_vtx, p.split_off):
        assert o == off and o % 32 == 0
        units = wg_bytes(lib, 0, 2, int(deg[v]) + 1, int(m[v]), bool(p.wg_box)) - wg_bytes(lib, 0, 2, 0, int(m[v]), bool(p.wg_box))
        off += -(-units // 256) * 32
    assert p.split_doubles == off


GRAPHS = [("benchmark" + str(i), lambda i=i: load_fixture("benchmark" + str(i))[1]) for i in (1, 2, 3, 4)] + [
    ("lattice 20x18", lambda: lattice_boxes(20, 18, seed=2)), ("lattice n=3", lambda: lattice_boxes(6, 5, n=3, seed=1)),
    ("lattice n=6", lambda: lattice_boxes(6, 5, n=6, seed=1)), ("star 40", lambda: star(40)),
    ("hub n=6 degree 16", lambda: hub_case(6, 8)), ("lattice 40x40", lambda: lattice_boxes(40, 40, seed=0))]


@pytest.mark.parametrize("name,mk", GRAPHS, ids=[c[0] for c in GRAPHS])
@pytest.mark.parametrize("knobs", [{}, dict(vertex_program=2), dict(vertex_program=3), dict(wave_generic_rows=1)], ids=["auto", "wg", "wg256", "generic"])
def test_graphs_that_fit_plan_identically_in_modes_0_and_1(lib, name, mk, knobs):
    g = mk()
    a, b = full_plan(lib, g, **knobs), full_plan(lib, g, vertex_workspace=1, **knobs)
    assert len(b.split_vtx) == 0 and b.split_doubles == 0 and b.split_lds_bytes == 0
    for k in a:
        if k in ("split_vtx", "split_off", "split_doubles", "split_lds_bytes"):
            continue
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name,mk", GRAPHS[:8], ids=[c[0] for c in GRAPHS[:8]])
def test_mode_2_moves_every_workgroup_vertex(lib, name, mk):
    g = mk()
    a, b = full_plan(lib, g), full_plan(lib, g, vertex_workspace=2)
    assert len(b.wg_vtx) == 0 and b.wg_lds_bytes == 0
    assert list(b.split_vtx) == list(a.wg_vtx)       # (heaviest first: the in-LDS launch's order)
    assert b.wg_box == a.wg_box and b.wg_t512 == a.wg_t512
    for k in ("wave_vtx", "wave_slot_ptr", "special_vtx", "warm_ptr", "lds_bytes"):
        assert np.array_equal(a[k], b[k]), k
    if len(a.wg_vtx):
        assert 0 < b.split_lds_bytes < a.wg_lds_bytes and b.split_doubles > 0


def test_bad_value_and_polytope_too_large(lib):
    g = lattice_boxes(4, 3, seed=1)
    for bad in (-1, 3, 7):
        assert refusal(lib, g, vertex_workspace=bad) == (BAD_ARG, "vertex_workspace must be 0, 1 or 2")
    # a vertex whose fixed block and polytope alone exceed LDS: n = 8 with a polytope of 2 200 facets
    As, bs = {}, {}
    n = 8
    from gcs_admm_amd.graph import convert_pt_to_polytope
    rng = np.random.default_rng(0)
    D = rng.standard_normal((2200, n)); D /= np.linalg.norm(D, axis=1, keepdims=True)
    E = np.vstack([np.eye(n), -np.eye(n)])
    As[0], bs[0] = np.vstack([E, D]), np.hstack([np.ones(2 * n), np.full(len(D), 2.0)])
    As[1], bs[1] = E, np.hstack([np.full(n, 1.5), np.full(n, -0.5)])
    As['s'], bs['s'] = convert_pt_to_polytope(np.full(n, 0.9)); As['t'], bs['t'] = convert_pt_to_polytope(np.full(n, 0.95))
    g = graph_from_sets(As, bs, n, edges=[('s', 1), (1, 0), (0, 1), (1, 't')])
    assert 8 * lib.plan_ws_emu_split_lds_doubles(n, 2 * n + 2200, 0) > 160 * KB
    assert refusal(lib, g)[0] == UNSUPPORTED and refusal(lib, g)[1] == OLD_MSG
    for mode in (1, 2):
        assert refusal(lib, g, vertex_workspace=mode) == (UNSUPPORTED, POLY_MSG)


def test_n2_facet_count_beyond_the_wavefront_program_goes_to_the_workgroup_program(lib):
    """mode 1: an n = 2 vertex with so many facets that the wavefront program cannot hold it even alone in a wavefront (mode 0: "facet
    count too large for LDS") is solved by the workgroup program instead -- in LDS while it fits there"""
    from gcs_admm_amd.graph import convert_pt_to_polytope
    g0 = lattice_boxes(40, 40, seed=0)          # > 1 024 generic vertices: the automatic rule puts the lattice on the wavefront program
    from gcs_admm_amd.graph import sets_of_graph
    As, bs = sets_of_graph(g0)
    As, bs = {k: np.array(v) for k, v in As.items()}, {k: np.array(v) for k, v in bs.items()}
    k0 = g0.keys[2 + 5 * 40 + 5]                 # one interior cell becomes a polygon of many facets (same box, tangent cuts)
    A, b = As[k0], bs[k0]
    c = 0.5 * (b[:2] - b[2:]); r = 0.5 * min(b[0] + b[2], b[1] + b[3])
    ang = np.linspace(0, 2 * np.pi, 100, endpoint=False)
    D = np.stack([np.cos(ang), np.sin(ang)], 1)
    As[k0], bs[k0] = np.vstack([A, D]), np.hstack([b, D @ c + r * 1.2])
    g = graph_from_sets(As, bs, 2, edges=list(g0.edges_as_keys()))
    v = g.keys.index(k0)
    assert refusal(lib, g) == (UNSUPPORTED, "facet count too large for LDS")
    p = full_plan(lib, g, vertex_workspace=1)
    assert list(p.wg_vtx) == [v] and len(p.split_vtx) == 0 and v not in set(p.wave_vtx)
    assert p.wave_mm == 4 and p.n_waves > 0
