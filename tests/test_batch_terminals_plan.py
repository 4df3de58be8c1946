"""What gcsadmm_batch_create_ex decides under GCSADMM_BATCH_TERMINALS, checked without a GPU: gcs_admm_amd/csrc/batch_plan.h compiled
for the host (tests/hostemu/batch_terminals_plan_emu.cpp beside the create-plan shim, same sizing objects).  Pinned here: the refusal
of a member with a terminal that is a region where the flag is not set, with today's text; its acceptance where it is; the terminal
groups -- one per (threads, work arrays in LDS or in the workspace), every terminal of a two-terminal member listed, the group's LDS
the largest member's -- against the members' own create plans; the flag values; every other refusal; three seeded errors in the
grouping that the checks reject; and the registers and scratch of the batch kernels against the solo kernels of the same
instantiation, from the compiler's resource remarks.  What the GPU computes with such a batch is checked by
test_gpu_batch_terminals.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_terminals_cases as bc
import hostemu_lib
import test_create_plan as cp
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import lattice_boxes
from gcs_admm_amd.native_build import build_library
from mutant_build import build_mutants

OK, BAD_ARG, UNSUPPORTED = cp.OK, cp.BAD_ARG, cp.UNSUPPORTED
LARGE, TERMINALS = 1, 4              # GCSADMM_BATCH_LARGE, GCSADMM_BATCH_TERMINALS
WG256 = dict(vertex_program=3)       # what a batch's members are created with
REGION_TEXT = "a terminal that is a region"
SOURCE = ("batch_terminals_plan_emu.cpp", [])


def prepare(lib):
    lib.term_emu_error.restype = C.c_char_p
    lib.term_emu_get.restype = lib.term_emu_member.restype = lib.term_emu_group.restype = C.c_double
    lib.term_emu_clear()
    return lib


@pytest.fixture(scope="module")
def lib():
    so = build_library(os.path.join(hostemu_lib.HOSTEMU, "libbatchterminalsplanemu.so"),
                       hostemu_lib.sources(hostemu_lib.SIZES + [SOURCE]), flags=hostemu_lib.FLAGS + [hostemu_lib.INCLUDE])
    return prepare(C.CDLL(so))


@pytest.fixture(scope="module")
def plan_lib():
    return cp.load(cp.build_lib())


EXTRA = bc.EXTRA


def add(lib, g, has_comm=0, **kw):
    d, keep = cp.descriptor(g, **{**WG256, **kw})
    i = lib.term_emu_add(C.byref(d), has_comm)
    assert i >= 0, lib.term_emu_error().decode()
    return i


def make(lib, idx, flags=TERMINALS):
    arr = (C.c_int * max(len(idx), 1))(*idx)
    st = lib.term_emu_make(arr, len(idx), flags)
    return st, lib.term_emu_error().decode()


def groups(lib):
    """the terminal groups of the last plan: [dict(threads, in_lds, lds_doubles, entries=[(member, terminal)])]"""
    out = []
    for k in range(int(lib.term_emu_get(b"term_groups"))):
        g = {f: int(lib.term_emu_group(f.encode(), k, 0)) for f in ("threads", "in_lds", "lds_doubles")}
        g["entries"] = [(int(lib.term_emu_group(b"member", k, a)), int(lib.term_emu_group(b"term", k, a)))
                        for a in range(int(lib.term_emu_group(b"entries", k, 0)))]
        out.append(g)
    return out


@pytest.fixture(scope="module")
def members(lib, plan_lib):
    """{name: (index in the emulation, the member's own Plan)} of the shared cases and of EXTRA; each plan says about its terminals
    what the case table states"""
    out = {}
    for name, (graph, want) in {**{k: (lambda k=k: bc.graph(k), v[1]) for k, v in bc.CASES.items()}, **EXTRA}.items():
        g = graph()
        p = cp.plan(plan_lib, g, **WG256)
        assert (p.n_term, p.term_threads, p.term_lds_doubles > 0) == want, (name, p.n_term, p.term_threads, p.term_lds_doubles)
        assert p.n_waves == 0 and p.wg_t512 == 0, name
        out[name] = (add(lib, g), p)
    return out


def want_groups(plans):
    """the rule restated: terminals in member order, then terminal order, one group per (threads, LDS or not) in order of first
    appearance; the group's LDS is the largest term_lds_doubles of its members"""
    out = []
    for i, p in enumerate(plans):
        key = (p.term_threads, int(p.term_lds_doubles > 0))
        for ti in range(p.n_term):
            g = next((g for g in out if (g["threads"], g["in_lds"]) == key), None)
            if g is None:
                g = dict(threads=key[0], in_lds=key[1], lds_doubles=0, entries=[])
                out.append(g)
            g["entries"].append((i, ti))
            g["lds_doubles"] = max(g["lds_doubles"], p.term_lds_doubles)
    return out


BATCHES = {                     # members of one space dimension each
    "n2": ["row", "scene1", "star2x33", "scene2"],
    "n2 largest last": ["scene2", "row", "scene1"],
    "n3": ["star3", "star3b"],
    "n6": ["star6", "simplex6"],
    "n8": ["star8", "star8b"],
}


def check_groups(lib, members, names):
    """the plan of the batch ``names`` equals the restated rule; returns the groups"""
    st, msg = make(lib, [members[k][0] for k in names])
    assert st == OK, msg
    plans = [members[k][1] for k in names]
    got = groups(lib)
    assert got == want_groups(plans), (names, got)
    assert sum(len(g["entries"]) for g in got) == sum(p.n_term for p in plans)
    assert len({(g["threads"], g["in_lds"]) for g in got}) == len(got) <= 4
    for g in got:
        assert g["entries"] == sorted(g["entries"])
        assert (g["lds_doubles"] > 0) == bool(g["in_lds"]) and 8 * g["lds_doubles"] <= 48 * 1024
    assert int(lib.term_emu_get(b"flags")) == TERMINALS and int(lib.term_emu_get(b"wave_groups")) == 0
    return got


def check_all(lib, members):
    seen = set()
    for names in BATCHES.values():
        seen |= {(g["threads"], g["in_lds"]) for g in check_groups(lib, members, names)}
    assert seen == {(64, 1), (256, 1), (64, 0), (256, 0)}       # every launch shape a batch can have appears


def test_refused_without_the_flag_accepted_with_it(lib, members):
    """without GCSADMM_BATCH_TERMINALS the refusal is today's, with and without GCSADMM_BATCH_LARGE; with it the member is accepted,
    alone and beside LARGE; flags 2, 3 and bits above 4 stay unknown"""
    plain = add(lib, load_fixture("benchmark1")[1])
    for name in ("row", "scene1", "star3", "star6"):
        m = members[name][0]
        for flags in (0, LARGE):
            assert make(lib, [m], flags) == (UNSUPPORTED, "member 0: " + REGION_TEXT)
            if name in ("row", "scene1"):
                assert make(lib, [plain, m], flags) == (UNSUPPORTED, "member 1: " + REGION_TEXT)
        for flags in (TERMINALS, TERMINALS | LARGE):
            assert make(lib, [m], flags) == (OK, "")
            assert int(lib.term_emu_get(b"flags")) == flags and int(lib.term_emu_get(b"term_groups")) == 1
    for flags in (2, 3, 6, 7, 8, 12, 1 << 31):
        assert make(lib, [members["row"][0]], flags) == (BAD_ARG, "unknown batch flag")
    assert make(lib, [plain, members["row"][0]], TERMINALS | LARGE) == (OK, "")


def test_terminal_groups(lib, members):
    """terminals land in groups by (threads, LDS or workspace); both terminals of a two-terminal member are listed; the group's LDS is
    the largest member's; all four launch shapes appear over the batches"""
    check_all(lib, members)
    got = check_groups(lib, members, BATCHES["n2"])
    assert [(g["threads"], g["in_lds"]) for g in got] == [(64, 1), (256, 1)]
    assert got[0]["entries"] == [(0, 0), (0, 1), (1, 0), (1, 1), (3, 0), (3, 1)] and got[1]["entries"] == [(2, 0)]
    lds = [members[k][1].term_lds_doubles for k in BATCHES["n2"]]
    assert got[0]["lds_doubles"] == max(lds[0], lds[1], lds[3]) == lds[1] > lds[0] and got[1]["lds_doubles"] == lds[2]
    # the largest member is not the first one of its group
    got = check_groups(lib, members, BATCHES["n2 largest last"])
    assert got[0]["lds_doubles"] == members["scene1"][1].term_lds_doubles > members["scene2"][1].term_lds_doubles
    got = check_groups(lib, members, BATCHES["n6"])
    assert [(g["threads"], g["in_lds"], g["lds_doubles"]) for g in got] == [(256, 0, 0), (64, 0, 0)]


def test_the_rest_of_the_plan_is_the_plain_batch(lib, members, plan_lib):
    """the flag adds the terminal groups and changes nothing else: members without region terminals plan the same launches with it,
    and a member with them gets the vertex and edge geometry of its own create plan"""
    graphs = [load_fixture(k)[1] for k in ("test1", "benchmark1", "benchmark4")]
    idx = [add(lib, g) for g in graphs]
    seen = []
    for flags in (0, TERMINALS):
        st, msg = make(lib, idx, flags)
        assert st == OK, msg
        seen.append([int(lib.term_emu_get(k)) for k in (b"count", b"n", b"dtype", b"box", b"vertex_grid_x", b"vertex_lds_bytes", b"edge_grid_x",
                                                        b"wave_groups", b"wg_members", b"term_groups")]
                    + [int(lib.term_emu_member(b"vertex_grid", i)) for i in range(3)])
    assert seen[0] == seen[1] and seen[0][9] == 0
    names = BATCHES["n2"]
    st, msg = make(lib, idx + [members[k][0] for k in names])
    assert st == OK, msg
    for i, k in enumerate(names):
        p = members[k][1]
        assert int(lib.term_emu_member(b"vertex_grid", 3 + i)) == len(p.wg_vtx) + -(-len(p.special_vtx) // 256)
        assert int(lib.term_emu_member(b"edge_blocks", 3 + i)) == p.edge_blocks
    assert [e for g in groups(lib) for e in g["entries"] if e[0] < 3] == []


def check_refusals(lib, members, flags):
    g1, g4 = load_fixture("benchmark1")[1], load_fixture("benchmark4")[1]
    a, r = add(lib, g1), members["row"][0]
    assert make(lib, [a, r], flags)[0] == OK
    assert make(lib, [], flags) == (BAD_ARG, "a batch needs at least one member")
    assert make(lib, [r, a, r], flags) == (BAD_ARG, "member 2: the handle appears twice in the batch")
    assert make(lib, [r, members["star3"][0]], flags) == (UNSUPPORTED, "member 1: members must share the space dimension n")
    assert make(lib, [r, add(lib, bc.graph("scene1"), dtype=1)], flags) == (UNSUPPORTED, "member 1: members must share the state_dtype")
    assert make(lib, [r, add(lib, bc.graph("scene1"), device=1)], flags) == (BAD_ARG, "member 1: members must be on the same device")
    assert make(lib, [add(lib, bc.graph("scene1"), vertex_program=0), r], flags) == (
        UNSUPPORTED, "member 0: the workgroup program runs with 512 threads (create the handle with vertex_program = 3)")
    assert make(lib, [r, add(lib, g4, vertex_program=3, vertex_workspace=2)], flags) == (
        UNSUPPORTED, "member 1: vertices in the split form of the workgroup program (vertex_workspace)")
    assert make(lib, [r, add(lib, bc.graph("row"), has_comm=1)], flags) == (
        UNSUPPORTED, "member 1: a communicator is attached (partitioned handles run their own loop)")
    wide = lattice_boxes(190, 190)
    # (without GCSADMM_BATCH_LARGE the rule on 512 workgroup vertices is checked first, and such a lattice has more)
    assert make(lib, [r, add(lib, wide)], flags)[1] == ("member 1: the edge step runs unrolled (a graph this large gains nothing from a batch)" if flags & LARGE
                                                        else "member 1: 512 or more workgroup-program vertices (slowest-first dispatch)")
    l3 = lattice_boxes(5, 5, n=3)
    assert make(lib, [add(lib, l3), add(lib, l3, wave_generic_rows=1)], flags) == (
        UNSUPPORTED, "member 1: members must share the BOX choice of the workgroup program (plan.wg_box)")
    assert make(lib, [members["star3"][0], add(lib, l3, wave_generic_rows=1)], flags) == (
        UNSUPPORTED, "member 1: members must share the BOX choice of the workgroup program (plan.wg_box)")
    if not flags & LARGE:
        assert make(lib, [r, add(lib, bc.graph("scene1"), vertex_program=1)], flags) == (
            UNSUPPORTED, "member 1: vertices on the wavefront program (create the handle with vertex_program = 3)")
        assert make(lib, [r, add(lib, lattice_boxes(24, 24))], flags) == (
            UNSUPPORTED, "member 1: 512 or more workgroup-program vertices (slowest-first dispatch)")


@pytest.mark.parametrize("flags", [TERMINALS, TERMINALS | LARGE])
def test_refusals_that_remain(lib, members, flags):
    """every other rule stands when the flag is set, with the status and text it has without it"""
    check_refusals(lib, members, flags)


def test_a_wavefront_member_with_region_terminals_under_both_flags(lib, plan_lib):
    """GCSADMM_BATCH_TERMINALS | GCSADMM_BATCH_LARGE: region_scene(1) on the wavefront program is in a wave group AND in a terminal group"""
    g = bc.graph("scene1")
    p = cp.plan(plan_lib, g, vertex_program=1)
    assert p.n_waves > 0 and p.n_term == 2
    w, m = add(lib, g, vertex_program=1), add(lib, bc.graph("row"))
    assert make(lib, [w, m], TERMINALS) == (UNSUPPORTED, "member 0: vertices on the wavefront program (create the handle with vertex_program = 3)")
    assert make(lib, [w, m], LARGE) == (UNSUPPORTED, "member 0: " + REGION_TEXT)
    assert make(lib, [w, m], TERMINALS | LARGE) == (OK, "")
    assert int(lib.term_emu_get(b"wave_groups")) == 1 and int(lib.term_emu_member(b"wave_grid", 0)) > 0
    assert groups(lib) == [dict(threads=64, in_lds=1, lds_doubles=p.term_lds_doubles, entries=[(0, 0), (0, 1), (1, 0), (1, 1)])]


# (anchor in batch_plan.h, replacement): each anchor occurs exactly once
MUTANTS = {
    "clean": [],
    "ignores_threads": [("return t.threads == p.term_threads && t.in_lds == in_lds;", "return t.in_lds == in_lds;")],
    "lds_of_first_member": [("g->lds_doubles = std::max(g->lds_doubles, p.term_lds_doubles);",
                             "if (g->member.size() == 1) g->lds_doubles = p.term_lds_doubles;")],
    "drops_second_terminal": [("for (int ti = 0; ti < p.n_term; ++ti) {", "for (int ti = 0; ti < std::min(p.n_term, 1); ++ti) {")],
}


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    *sizes, (source, _) = hostemu_lib.sources(hostemu_lib.SIZES + [SOURCE])
    libs = build_mutants(tmp_path_factory.mktemp("batch_terminals_mutants"), "batch_plan.h", MUTANTS, source, flags=[hostemu_lib.INCLUDE], more=sizes)
    return {k: prepare(v) for k, v in libs.items()}


def mutant_members(lib, members):
    """the same members, added to the mutant's own emulation in the same order: {name: (index, plan)}"""
    out = {}
    for name in list(bc.CASES) + list(EXTRA):
        out[name] = (add(lib, EXTRA[name][0]() if name in EXTRA else bc.graph(name)), members[name][1])
    return out


def test_clean_copy_passes(builds, members):
    check_all(builds["clean"], mutant_members(builds["clean"], members))


@pytest.mark.parametrize("mutant,batch", [("ignores_threads", "n2"), ("lds_of_first_member", "n2 largest last"), ("drops_second_terminal", "n2")])
def test_seeded_errors_are_rejected(builds, members, mutant, batch):
    """grouping that ignores the thread count, LDS taken from the first member instead of the largest, a terminal of a two-terminal
    member dropped: each fails the comparison with the restated rule on the named batch"""
    lib = builds[mutant]
    with pytest.raises(AssertionError):
        check_groups(lib, mutant_members(lib, members), BATCHES[batch])


def _instantiation(name):
    m = re.search(r"terminal_region_(batch_)?kernelILi(\d)E([df])Lb([01])E", name)
    return m and (bool(m.group(1)), (int(m.group(2)), m.group(3), int(m.group(4))))


def test_batch_terminal_kernels_cost_no_residency():
    """terminal_region_batch_kernel reads its arguments from a table instead of the kernarg segment.  All 32 instantiations -- n = 1 ..
    8 x {f64, f32} x LDSWS -- are in the build beside the 32 solo kernels; none uses scratch; each needs no more VGPRs (the compiler's
    VGPRs remark) than the solo kernel of the same <N, T, LDSWS> and, with its AGPRs, fits the 512 registers of a lane as that one
    does, at the same occupancy.  (profiles/batch_terminals/README.md has the table; AGPRs are where this compiler keeps what would
    spill, and they differ by a few either way between the two kernels.)"""
    from gcs_admm_amd import build
    res = build.kernel_resources()
    solo, batch = {}, {}
    for k, v in res.items():
        inst = _instantiation(k)
        if inst:
            (batch if inst[0] else solo)[inst[1]] = v
    want = {(n, t, l) for n in range(1, 9) for t in "df" for l in (0, 1)}
    assert set(solo) == set(batch) == want
    for key in sorted(want):
        s, b = solo[key], batch[key]
        assert b["scratch"] == 0 and s["scratch"] == 0, (key, b)
        assert b["vgprs"] <= s["vgprs"], (key, b, s)
        assert b["vgprs"] + b["agprs"] <= 512, (key, b)
        assert b["lds"] == s["lds"], (key, b, s)
        # registers per lane decide how many workgroups a SIMD holds: the batch kernel is in the solo kernel's class (128: 4, 168: 3, 256: 2, 512: 1)
        tier = lambda r: next(t for t in (128, 168, 256, 512) if r["vgprs"] + r["agprs"] <= t)
        assert tier(b) <= tier(s), (key, b, s)
