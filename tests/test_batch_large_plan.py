"""What gcsadmm_batch_create_ex decides under GCSADMM_BATCH_LARGE, checked without a GPU: gcs_admm_amd/csrc/batch_plan.h compiled for
the host with its flags (tests/hostemu/batch_large_plan_emu.cpp beside the create-plan shim, same sizing objects).  Pinned here: the
members' own wavefront plans the launches are made of, the two refusals the flag lifts (with the flag and without), the wave groups
with every grid and LDS size against the maxima of the members' plans restated in numpy, the rows of the workgroup launch, every
refusal that remains with its message, and the registers and scratch of the sixteen wave batch kernels from the compiler's resource
remarks.  What the GPU computes with such a batch is checked by test_gpu_batch_large.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostemu_lib
import test_create_plan as cp
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import lattice_boxes
from gcs_admm_amd.native_build import build_library
from test_gpu_configs import _region_star

OK, BAD_ARG, UNSUPPORTED = cp.OK, cp.BAD_ARG, cp.UNSUPPORTED
LARGE = 1                            # GCSADMM_BATCH_LARGE
WAVE = dict(vertex_program=1)        # what solver.DeviceSolver(program="wavefront") asks for
WG256 = dict(vertex_program=3)
MAX_SPECIAL_DEG = 256                # step_args.h
FLOOR = 4 * MAX_SPECIAL_DEG * 8      # the work arrays of the closed-form workgroups
WAVE_TEXT = "vertices on the wavefront program (create the handle with vertex_program = 3)"
REORDER_TEXT = "512 or more workgroup-program vertices (slowest-first dispatch)"


@pytest.fixture(scope="module")
def lib():
    so = build_library(os.path.join(hostemu_lib.HOSTEMU, "libbatchlargeplanemu.so"),
                       hostemu_lib.sources(hostemu_lib.SIZES + [("batch_large_plan_emu.cpp", [])]), flags=hostemu_lib.FLAGS + [hostemu_lib.INCLUDE])
    lib = C.CDLL(so)
    lib.large_emu_error.restype = C.c_char_p
    lib.large_emu_get.restype = lib.large_emu_member.restype = lib.large_emu_group.restype = C.c_double
    lib.large_emu_clear()
    return lib


@pytest.fixture(scope="module")
def plan_lib():
    return cp.load(cp.build_lib())


def fixture_graph(name):
    return load_fixture(name)[1]


def mixed_graph(hubs=256, fan=33, chain=12, seed=0):
    """One graph with both kinds of generic vertices at n = 2: ``hubs`` hub boxes and as many leaf boxes, hub h joined both ways to
    the leaves h .. h + fan - 1 (cyclically), so all of them have 2 fan = 66 incident edges, more than a wavefront holds; and a chain
    of ``chain`` boxes of 4 incident edges from s to hub 0, which the wavefront program takes.  t hangs on leaf 0.  Every box is a unit
    box around a point within 0.2 of the origin, so every edge joins two boxes that overlap.  512 workgroup vertices: more than 255, or
    the workgroup program would run with 512 threads and the batch would refuse the member for that."""
    from gcs_admm_amd.graph import convert_pt_to_polytope, graph_from_sets
    rng = np.random.default_rng(seed)
    A = np.vstack([np.eye(2), -np.eye(2)])
    As, bs, edges = {}, {}, []
    As["s"], bs["s"] = convert_pt_to_polytope(np.array([-0.3, 0.1]))
    As["t"], bs["t"] = convert_pt_to_polytope(np.array([0.3, -0.1]))
    for kind, count in (("hub", hubs), ("leaf", hubs), ("chain", chain)):
        for i in range(count):
            c = rng.uniform(-0.2, 0.2, 2)
            As[(kind, i)], bs[(kind, i)] = A, np.hstack([c + 0.5, -(c - 0.5)])
    both = lambda u, w: [(u, w), (w, u)]
    for h in range(hubs):
        for j in range(fan):
            edges += both(("hub", h), ("leaf", (h + j) % hubs))
    edges += [("s", ("chain", 0))]
    for i in range(chain - 1):
        edges += both(("chain", i), ("chain", i + 1))
    edges += both(("chain", chain - 1), ("hub", 0)) + [(("leaf", 0), "t")]
    return graph_from_sets(As, bs, 2, edges=edges)


def add(lib, g, has_comm=0, **kw):
    """a member made from the descriptor DeviceSolver would hand to gcsadmm_create (default: program="wavefront"); its index"""
    d, keep = cp.descriptor(g, **{**WAVE, **kw})
    i = lib.large_emu_add(C.byref(d), has_comm)
    assert i >= 0, lib.large_emu_error().decode()
    return i


def make(lib, idx, flags=LARGE):
    arr = (C.c_int * max(len(idx), 1))(*idx)
    st = lib.large_emu_make(arr, len(idx), flags)
    return st, lib.large_emu_error().decode()


def groups(lib):
    """the wave groups of the last plan: [dict(all_m4, align_rows, store_dl, grid_x, lds_bytes, members)]"""
    out = []
    for k in range(int(lib.large_emu_get(b"wave_groups"))):
        g = {f: int(lib.large_emu_group(f.encode(), k, 0)) for f in ("all_m4", "align_rows", "store_dl", "grid_x", "lds_bytes")}
        g["members"] = [int(lib.large_emu_group(b"member", k, a)) for a in range(int(lib.large_emu_group(b"members", k, 0)))]
        out.append(g)
    return out


def wg_rows(lib):
    return [int(lib.large_emu_member(b"wg_member", a)) for a in range(int(lib.large_emu_get(b"wg_members")))]


# (graph, knobs beside vertex_program = 1) -> what the member's own plan must say (create_plan.h's packing and LDS rules on these graphs)
GENERIC, BOX = 0, 2
L12 = lambda: lattice_boxes(12, 12)
CASES = {
    "test1": (lambda: fixture_graph("test1"), {}, dict(n_waves=1, all_m4=GENERIC, align_rows=1, store_dl=1, lds_bytes=15664)),
    "benchmark1": (lambda: fixture_graph("benchmark1"), {}, dict(n_waves=4, all_m4=GENERIC, lds_bytes=19792)),
    "benchmark4": (lambda: fixture_graph("benchmark4"), {}, dict(n_waves=39, all_m4=GENERIC, lds_bytes=32144)),
    "3x3": (lambda: lattice_boxes(3, 3), {}, dict(n_waves=9, all_m4=BOX, lds_bytes=15696)),
    "5x4": (lambda: lattice_boxes(5, 4), {}, dict(n_waves=20, all_m4=BOX)),
    "12x12": (L12, {}, dict(n_waves=144, all_m4=BOX, edge_blocks=2)),
    "12x12 dense": (L12, dict(wave_align=2), dict(all_m4=BOX, align_rows=0)),
    "12x12 no dl": (L12, dict(wave_store_dl=2), dict(all_m4=BOX, store_dl=0, lds_bytes=7504)),
    "12x12 generic": (L12, dict(wave_generic_rows=1), dict(all_m4=GENERIC)),
    "25x40": (lambda: lattice_boxes(25, 40), {}, dict(n_waves=1000, wave_reorder=1)),
}


@pytest.fixture(scope="module")
def members(lib, plan_lib):
    """{name: (index in the emulation, the member's own Plan)} of CASES, and the 24 x 24 workgroup member"""
    out = {}
    for name, (graph, knobs, want) in CASES.items():
        g = graph()
        p = cp.plan(plan_lib, g, **{**WAVE, **knobs})
        assert {k: p[k] for k in want} == want, name
        assert len(p.wg_vtx) == 0 and p.n_waves > 0, name
        out[name] = (add(lib, g, **knobs), p)
    big = lattice_boxes(24, 24)
    p = cp.plan(plan_lib, big, **WG256)
    assert len(p.wg_vtx) == 576 and p.n_waves == 0 and p.wg_reorder == 1
    out["24x24 wg"] = (add(lib, big, **WG256), p)
    return out


def test_flag_lifts_the_two_limits(lib, members):
    """without the flag a wavefront member and a member of 512 or more workgroup vertices are refused with today's texts; with it both
    are members; a flag bit nobody defined is BAD_ARG"""
    wave, big = members["benchmark1"][0], members["24x24 wg"][0]
    assert make(lib, [wave], 0) == (UNSUPPORTED, "member 0: " + WAVE_TEXT)
    assert make(lib, [big], 0) == (UNSUPPORTED, "member 0: " + REORDER_TEXT)
    assert make(lib, [members["25x40"][0]], 0) == (UNSUPPORTED, "member 0: " + WAVE_TEXT)
    assert make(lib, [wave]) == (OK, "") and make(lib, [big]) == (OK, "") and make(lib, [big, wave, members["25x40"][0]]) == (OK, "")
    assert int(lib.large_emu_get(b"flags")) == LARGE
    for flags in (2, 3, 1 << 31):
        assert make(lib, [wave], flags) == (BAD_ARG, "unknown batch flag")


def test_wave_groups(lib, members):
    """members that share (all_m4, align_rows, store_dl) share a launch: the three fixtures one, the three lattices one, every knob
    variant of the 12 x 12 lattice one of its own; grid (max grid_x, members) and LDS max(lds_bytes, floor) over the group"""
    names = ["test1", "3x3", "benchmark1", "12x12 dense", "5x4", "benchmark4", "12x12", "12x12 no dl", "12x12 generic"]
    idx = [members[k][0] for k in names]
    plans = [members[k][1] for k in names]
    st, msg = make(lib, idx)
    assert st == OK, msg
    at = {k: i for i, k in enumerate(names)}
    want = [[at[k] for k in ks] for ks in (["test1", "benchmark1", "benchmark4"], ["3x3", "5x4", "12x12"], ["12x12 dense"], ["12x12 no dl"])]
    got = groups(lib)
    # 12x12 generic: generic rows, aligned, stored directions -- the instantiation of the fixtures, so it joins their group
    generic = plans[at["12x12 generic"]]
    assert (generic.all_m4, generic.align_rows, generic.store_dl) == (GENERIC, 1, 1)
    want[0].append(at["12x12 generic"])
    assert sorted(g["members"] for g in got) == sorted(want)
    grid = np.array([p.n_waves + -(-len(p.special_vtx) // 64) for p in plans])
    lds = np.array([max(p.lds_bytes, FLOOR) for p in plans])
    assert len(set(grid)) > 3 and len(set(lds)) > 3
    for g in got:
        m = g["members"]
        assert m == sorted(m)
        assert {(plans[i].all_m4, plans[i].align_rows, plans[i].store_dl) for i in m} == {(g["all_m4"], g["align_rows"], g["store_dl"])}
        assert g["grid_x"] == grid[m].max() and g["lds_bytes"] == lds[m].max(), g
    assert len({(g["all_m4"], g["align_rows"], g["store_dl"]) for g in got}) == len(got)
    for i in range(len(names)):
        assert int(lib.large_emu_member(b"wave_grid", i)) == grid[i]
        assert int(lib.large_emu_member(b"vertex_grid", i)) == 0          # the closed-form vertices ride on the wave launch
        assert int(lib.large_emu_member(b"edge_blocks", i)) == plans[i].edge_blocks
    # no member has anything in the workgroup launch: there is none
    assert wg_rows(lib) == [] and int(lib.large_emu_get(b"vertex_grid_x")) == 0
    assert int(lib.large_emu_get(b"edge_grid_x")) == max(p.edge_blocks for p in plans) == 2


def test_the_generic_rows_variant_is_a_group_of_its_own_beside_the_lattices(lib, members):
    """the four 12 x 12 members alone: box aligned, box dense, box without stored directions, generic -- four launches"""
    names = ["12x12", "12x12 dense", "12x12 no dl", "12x12 generic"]
    st, msg = make(lib, [members[k][0] for k in names])
    assert st == OK, msg
    got = groups(lib)
    assert [g["members"] for g in got] == [[0], [1], [2], [3]]
    assert [(g["all_m4"], g["align_rows"], g["store_dl"]) for g in got] == [(BOX, 1, 1), (BOX, 0, 1), (BOX, 1, 0), (GENERIC, 1, 1)]
    assert got[2]["lds_bytes"] == FLOOR > members["12x12 no dl"][1].lds_bytes == 7504


def test_mixed_batch(lib, plan_lib, members):
    """wavefront members beside workgroup members: the workgroup launch has rows for the members with something in it alone, its grid
    and LDS are theirs, and a workgroup member keeps its closed-form vertices there"""
    g4 = fixture_graph("benchmark4")
    p4 = cp.plan(plan_lib, g4, **WG256)
    small = add(lib, g4, **WG256)
    idx = [members["12x12"][0], small, members["5x4"][0], members["24x24 wg"][0]]
    st, msg = make(lib, idx)
    assert st == OK, msg
    assert wg_rows(lib) == [1, 3]
    big = members["24x24 wg"][1]
    grid = [len(p.wg_vtx) + -(-len(p.special_vtx) // 256) for p in (p4, big)]
    assert [int(lib.large_emu_member(b"vertex_grid", i)) for i in range(4)] == [0, grid[0], 0, grid[1]]
    assert int(lib.large_emu_get(b"vertex_grid_x")) == max(grid) == 577
    assert int(lib.large_emu_get(b"vertex_lds_bytes")) == max(max(p.wg_lds_bytes, FLOOR) for p in (p4, big))
    assert [g["members"] for g in groups(lib)] == [[0, 2]]
    assert [int(lib.large_emu_member(b"wave_grid", i)) for i in range(4)] == [145, 0, 21, 0]
    assert int(lib.large_emu_get(b"box")) == 0 and int(lib.large_emu_get(b"count")) == 4


def test_one_member_with_both_kinds_of_vertices(lib, plan_lib, members):
    """512 vertices of degree 66 on the workgroup program and a chain of 12 on the wavefront program in ONE handle: its workgroup
    vertices are a row of the workgroup launch, without closed-form workgroups, and its closed-form vertices ride on its wave launch"""
    g = mixed_graph()
    p = cp.plan(plan_lib, g, **WAVE)
    assert len(p.wg_vtx) == 512 and p.n_waves == 12 and len(p.special_vtx) == 2 and p.wg_t512 == 0 and p.all_m4 == BOX and p.wg_box == 0
    m = add(lib, g)
    assert make(lib, [m], 0) == (UNSUPPORTED, "member 0: " + WAVE_TEXT)
    st, msg = make(lib, [members["5x4"][0], m, members["24x24 wg"][0]])
    assert st == OK, msg
    assert wg_rows(lib) == [1, 2]
    assert [int(lib.large_emu_member(b"vertex_grid", i)) for i in range(3)] == [0, 512, 577]
    assert [int(lib.large_emu_member(b"wave_grid", i)) for i in range(3)] == [21, 13, 0]
    assert int(lib.large_emu_get(b"vertex_grid_x")) == 577
    assert int(lib.large_emu_get(b"vertex_lds_bytes")) == max(p.wg_lds_bytes, members["24x24 wg"][1].wg_lds_bytes, FLOOR) == p.wg_lds_bytes
    got = groups(lib)
    assert [g_["members"] for g_ in got] == [[0, 1]] and got[0]["grid_x"] == 21
    assert got[0]["lds_bytes"] == max(members["5x4"][1].lds_bytes, p.lds_bytes, FLOOR)


def test_flag_changes_nothing_for_plain_members(lib, plan_lib):
    """a batch of workgroup256 members plans the same launch with the flag as without"""
    graphs = [fixture_graph("test1"), fixture_graph("benchmark1"), fixture_graph("benchmark4"), lattice_boxes(12, 12)]
    idx = [add(lib, g, **WG256) for g in graphs]
    seen = []
    for flags in (0, LARGE):
        st, msg = make(lib, idx, flags)
        assert st == OK, msg
        seen.append(([int(lib.large_emu_get(k)) for k in (b"count", b"n", b"dtype", b"box", b"vertex_grid_x", b"vertex_lds_bytes", b"edge_grid_x", b"wave_groups")],
                     wg_rows(lib), [int(lib.large_emu_member(b"vertex_grid", i)) for i in range(4)], [int(lib.large_emu_member(b"wave_grid", i)) for i in range(4)]))
    assert seen[0] == seen[1] and seen[0][1] == [0, 1, 2, 3] and seen[0][3] == [0] * 4 and seen[0][0][-1] == 0


def test_refusals_that_remain(lib, members):
    """every rule the flag does not lift, with the status and text it has without the flag"""
    g1, g4 = fixture_graph("benchmark1"), fixture_graph("benchmark4")
    a, b = members["benchmark1"][0], members["benchmark4"][0]
    assert make(lib, [a, b])[0] == OK
    assert make(lib, []) == (BAD_ARG, "a batch needs at least one member")
    assert make(lib, [a, b, a]) == (BAD_ARG, "member 2: the handle appears twice in the batch")
    assert make(lib, [a, add(lib, lattice_boxes(5, 5, n=3), **WG256)]) == (UNSUPPORTED, "member 1: members must share the space dimension n")
    assert make(lib, [a, add(lib, g4, dtype=1)]) == (UNSUPPORTED, "member 1: members must share the state_dtype")
    assert make(lib, [a, add(lib, g4, device=1)]) == (BAD_ARG, "member 1: members must be on the same device")
    assert make(lib, [add(lib, g4, vertex_program=0), a]) == (
        UNSUPPORTED, "member 0: the workgroup program runs with 512 threads (create the handle with vertex_program = 3)")
    assert make(lib, [a, b, add(lib, g4, vertex_program=3, vertex_workspace=2)]) == (
        UNSUPPORTED, "member 2: vertices in the split form of the workgroup program (vertex_workspace)")
    assert make(lib, [add(lib, _region_star(3, 8, seed=3), **WG256)]) == (UNSUPPORTED, "member 0: a terminal that is a region")
    assert make(lib, [a, add(lib, g1, has_comm=1)]) == (
        UNSUPPORTED, "member 1: a communicator is attached (partitioned handles run their own loop)")
    # 131 072 edges and more run two edges per thread at f64: the unrolled edge kernel has no batch form
    wide = lattice_boxes(190, 190)
    assert wide.num_edges >= 131072
    unrolled = add(lib, wide)
    assert make(lib, [a, unrolled]) == (UNSUPPORTED, "member 1: the edge step runs unrolled (a graph this large gains nothing from a batch)")
    assert make(lib, [add(lib, wide, **WG256)])[1] == "member 0: the edge step runs unrolled (a graph this large gains nothing from a batch)"
    # the BOX choice binds the members that have workgroup vertices: two n = 3 lattices, one of them on generic rows
    l3 = lattice_boxes(5, 5, n=3)
    assert make(lib, [add(lib, l3, **WG256), add(lib, l3, vertex_program=3, wave_generic_rows=1)]) == (
        UNSUPPORTED, "member 1: members must share the BOX choice of the workgroup program (plan.wg_box)")


def test_wave_batch_kernels_fit_the_register_file():
    """all sixteen instantiations -- {generic, box} x {f64, f32} x RMODE x SDL -- are in the build, none uses scratch, and each fits
    the register file of a SIMD (512 per lane): the one-wavefront-per-SIMD residency of the solo kernel"""
    from gcs_admm_amd import build
    res = build.kernel_resources()
    batch = {k: v for k, v in res.items() if "vertex_wave_batch_kernel" in k}
    assert len(batch) == 16, sorted(batch)
    for prog in ("ProgGeneric", "ProgBox"):
        for t in "df":
            for rmode in (0, 1):
                for sdl in (0, 1):
                    assert any(f"{prog}ELi2E{t}Li{rmode}ELi{sdl}E" in k for k in batch), (prog, t, rmode, sdl)
    for k, v in batch.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgprs"] + v["agprs"] <= 512, (k, v)
