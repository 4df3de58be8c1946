"""What gcsadmm_batch_create decides, checked without a GPU: gcs_admm_amd/csrc/batch_plan.h compiled for the host
(tests/hostemu/batch_plan_emu.cpp beside the create-plan shim, same sizing objects).  Pinned here: the launch geometry of a batch
against the maxima of its members' own plans (those come from the create-plan shim of test_create_plan.py, restated in numpy), every
refusal with its message, and the registers and scratch of the two batch kernels from the compiler's resource remarks.  What the GPU
computes with a batch is checked by test_gpu_batch.py."""
import ctypes as C

import numpy as np
import pytest

import test_create_plan as cp
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import lattice_boxes
from hostemu_lib import emu_library
from test_gpu_configs import _region_star

OK, BAD_ARG, UNSUPPORTED = cp.OK, cp.BAD_ARG, cp.UNSUPPORTED
WG256 = dict(vertex_program=3)       # what solver.DeviceSolver(program="workgroup256") asks for: the program a batch member runs
MAX_SPECIAL_DEG = 256                # step_args.h


@pytest.fixture(scope="module")
def lib():
    lib = emu_library("batchplanemu")
    lib.batch_emu_error.restype = C.c_char_p
    lib.batch_emu_get.restype = lib.batch_emu_member.restype = C.c_double
    return lib


@pytest.fixture(scope="module")
def plan_lib():
    return cp.load(cp.build_lib())


def add(lib, g, has_comm=0, **kw):
    """a member made from the descriptor DeviceSolver would hand to gcsadmm_create (default: program="workgroup256"); its index"""
    d, keep = cp.descriptor(g, **{**WG256, **kw})
    i = lib.batch_emu_add(C.byref(d), has_comm)
    assert i >= 0, lib.batch_emu_error().decode()
    return i


def make(lib, idx):
    arr = (C.c_int * max(len(idx), 1))(*idx)
    st = lib.batch_emu_make(arr, len(idx))
    return st, lib.batch_emu_error().decode()


def test_geometry_is_the_maximum_over_the_members(lib, plan_lib):
    """vertex grid (max_m(n_vtx_m + ceil(n_special_m / 256)), count), dynamic LDS max_m(max(wg_lds_bytes_m, 4 MAX_SPECIAL_DEG 8)), edge
    grid (max_m edge_blocks_m, count) -- with every member's own extent recorded for its table entry"""
    lib.batch_emu_clear()
    graphs = [load_fixture("test1")[1], load_fixture("benchmark1")[1], load_fixture("benchmark4")[1], lattice_boxes(12, 12)]
    idx = [add(lib, g) for g in graphs]
    st, msg = make(lib, idx)
    assert st == OK, msg
    plans = [cp.plan(plan_lib, g, **WG256) for g in graphs]
    for p, g in zip(plans, graphs):
        assert p.wg_t512 == 0 and p.n_waves == 0 and p.n_term == 0 and p.edge_unroll == 1 and len(p.wg_vtx) == len(cp.generic(g))
    grid = np.array([len(p.wg_vtx) + -(-len(p.special_vtx) // 256) for p in plans])
    lds = np.array([max(p.wg_lds_bytes, 4 * MAX_SPECIAL_DEG * 8) for p in plans])
    eb = np.array([p.edge_blocks for p in plans])
    assert eb[3] > 1 and np.all(eb[:3] == 1)          # the lattice has more than 256 edges: the multi-workgroup edge step is in the batch
    assert len(set(grid)) > 1 and len(set(lds)) > 1   # the maxima are of different members' numbers
    got = {k: int(lib.batch_emu_get(k.encode())) for k in ("count", "n", "dtype", "device", "box", "vertex_grid_x", "vertex_lds_bytes", "edge_grid_x")}
    assert got == dict(count=4, n=2, dtype=0, device=0, box=0, vertex_grid_x=int(grid.max()), vertex_lds_bytes=int(lds.max()),
                       edge_grid_x=int(eb.max()))
    for m, i in enumerate(idx):
        assert int(lib.batch_emu_member(b"vertex_grid", m, i)) == grid[m]
        assert int(lib.batch_emu_member(b"edge_blocks", m, i)) == eb[m]
    # a batch of one is the member's own launch; the order of the members is kept
    st, msg = make(lib, [idx[2]])
    assert st == OK and int(lib.batch_emu_get(b"vertex_grid_x")) == grid[2] and int(lib.batch_emu_get(b"vertex_lds_bytes")) == lds[2]
    st, msg = make(lib, idx[::-1])
    assert st == OK and [int(lib.batch_emu_member(b"vertex_grid", m, 0)) for m in range(4)] == list(grid[::-1])


def test_box_batch(lib, plan_lib):
    """n = 3 box lattices: the BOX instantiation serves the launch when every member chose it"""
    lib.batch_emu_clear()
    graphs = [lattice_boxes(5, 5, n=3, seed=s) for s in range(3)]
    idx = [add(lib, g) for g in graphs]
    st, msg = make(lib, idx)
    assert st == OK, msg
    assert int(lib.batch_emu_get(b"box")) == 1 and int(lib.batch_emu_get(b"n")) == 3
    assert int(lib.batch_emu_get(b"vertex_lds_bytes")) == max(max(cp.plan(plan_lib, g, **WG256).wg_lds_bytes, 8192) for g in graphs)
    # one member on the generic instantiation: no common kernel
    generic_rows = add(lib, graphs[0], wave_generic_rows=1)
    assert make(lib, idx + [generic_rows]) == (UNSUPPORTED, "member 3: members must share the BOX choice of the workgroup program (plan.wg_box)")


def test_refusals(lib):
    """every rule with its status and the text that names the member and the reason"""
    lib.batch_emu_clear()
    g1, g4 = load_fixture("benchmark1")[1], load_fixture("benchmark4")[1]
    a, b = add(lib, g1), add(lib, g4)
    assert make(lib, [a, b])[0] == OK
    assert make(lib, []) == (BAD_ARG, "a batch needs at least one member")
    assert make(lib, [a, b, a]) == (BAD_ARG, "member 2: the handle appears twice in the batch")
    assert make(lib, [a, add(lib, lattice_boxes(5, 5, n=3))]) == (UNSUPPORTED, "member 1: members must share the space dimension n")
    assert make(lib, [a, add(lib, g4, dtype=1)]) == (UNSUPPORTED, "member 1: members must share the state_dtype")
    assert make(lib, [a, add(lib, g4, device=1)]) == (BAD_ARG, "member 1: members must be on the same device")
    # the automatic plan of a small graph runs 512 threads per workgroup
    assert make(lib, [add(lib, g4, vertex_program=0), a]) == (
        UNSUPPORTED, "member 0: the workgroup program runs with 512 threads (create the handle with vertex_program = 3)")
    assert make(lib, [a, add(lib, g4, vertex_program=1)]) == (
        UNSUPPORTED, "member 1: vertices on the wavefront program (create the handle with vertex_program = 3)")
    assert make(lib, [a, b, add(lib, g4, vertex_workspace=2)]) == (
        UNSUPPORTED, "member 2: vertices in the split form of the workgroup program (vertex_workspace)")
    assert make(lib, [add(lib, _region_star(3, 8, seed=3))]) == (UNSUPPORTED, "member 0: a terminal that is a region")
    assert make(lib, [a, add(lib, g4, has_comm=1)]) == (
        UNSUPPORTED, "member 1: a communicator is attached (partitioned handles run their own loop)")
    # 512 generic vertices or more: the handle keeps a slowest-first reorder buffer
    big = lattice_boxes(24, 24)
    assert len(cp.generic(big)) >= 512
    assert make(lib, [a, add(lib, big)]) == (UNSUPPORTED, "member 1: 512 or more workgroup-program vertices (slowest-first dispatch)")
    # the first violation in member order is the one reported
    assert make(lib, [a, add(lib, g4, vertex_program=1), add(lib, g4, dtype=1)])[1].startswith("member 1: vertices on the wavefront program")


def test_batch_kernels_fit_the_register_file():
    """The batch kernels read their arguments from a table instead of the kernarg segment.  That must not cost residency: registers
    within the bounds test_build.py sets for the solo kernels (n = 2, 3: <= 128, four workgroups per CU; n = 6: <= 256, its BOX form <=
    168) and no scratch anywhere; the 512-thread objects have no batch form."""
    from gcs_admm_amd import build
    res = build.kernel_resources()
    batch = {k: v for k, v in res.items() if "vertex_wg_batch_kernel" in k}
    for n in (2, 3, 6):
        assert any(f"vertex_wg_batch_kernelILi{n}E" in k for k in batch), n
    assert not any("gcs_wg_t512" in k for k in batch)
    edge = {k: v for k, v in res.items() if "edge_batch_kernel" in k}
    assert len(edge) == 16 and any("batch_poll_kernel" in k for k in res)          # {f64, f32} x c = 3 .. 17
    for k, v in {**batch, **edge}.items():
        assert v["scratch"] == 0, (k, v)
    for k, v in batch.items():
        regs = v["vgprs"] + v["agprs"]
        if "kernelILi2E" in k or "kernelILi3E" in k:
            assert regs <= 128, (k, v)
        if "kernelILi6E" in k:
            assert regs <= (168 if "Lb1E" in k else 256), (k, v)
