"""When gcsadmm_run runs an iteration as ONE launch (CreatePlan::fused_tail, gcs_admm_amd/csrc/create_plan.h), decided on the host and
checked without a GPU, the way test_create_plan.py reaches make_create_plan (tests/hostemu/fused_plan_emu.cpp): the rule -- all edges
in one edge workgroup, every generic vertex on the in-LDS workgroup program, no region terminal, a whole (unpartitioned) handle -- case
by case, and the LDS request of the launch that carries the tail."""
import ctypes as C

import numpy as np
import pytest

from fused_tail_cases import EDGE_BLOCK, largest_fused_lattice, path3, smallest_unfused_lattice
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import lattice_boxes
from hostemu_lib import emu_library
from test_create_plan import descriptor


@pytest.fixture(scope="module")
def lib():
    lib = emu_library("fusedplanemu")
    lib.fused_plan_error.restype = C.c_char_p
    return lib


def plan(lib, g, **kw):
    d, keep = descriptor(g, **kw)
    st = lib.fused_plan_make(C.byref(d))
    assert st == 0, lib.fused_plan_error().decode()
    names = ("fused_tail", "edge_blocks", "n_waves", "n_wg", "n_split", "n_term", "wg_t512", "wg_lds_bytes", "launch_lds_bytes",
             "tail_lds_bytes", "edge_block")
    return {k: lib.fused_plan_get(k.encode()) for k in names}


def test_small_graphs_fuse(lib):
    """benchmark4 (the headline of bench.py) and a 3 x 3 box lattice: one launch per iteration, in either state type and at either
    thread count of the workgroup program"""
    _, b4 = load_fixture("benchmark4")
    for g in (b4, lattice_boxes(3, 3)):
        for kw in ({}, {"dtype": 1}, {"vertex_program": 3}, {"vertex_program": 2}, {"columns": "edge"}):
            p = plan(lib, g, **kw)
            assert p["fused_tail"] == 1 and p["edge_blocks"] == 1 and p["n_waves"] == 0 and p["n_wg"] > 0, (kw, p)
    assert plan(lib, b4)["wg_t512"] == 1 and plan(lib, b4, vertex_program=3)["wg_t512"] == 0


def test_edge_count_decides(lib):
    """exactly EDGE_BLOCK edges still fuse (the last edge thread is in use), one lattice further does not; the fusing lattice forced
    onto the wavefront program does not either"""
    assert plan(lib, path3())["edge_block"] == EDGE_BLOCK
    big = largest_fused_lattice()
    assert big.num_edges == EDGE_BLOCK
    p = plan(lib, big)
    assert p["fused_tail"] == 1 and p["edge_blocks"] == 1, p
    over = smallest_unfused_lattice()
    assert over.num_edges > EDGE_BLOCK
    p = plan(lib, over)
    assert p["fused_tail"] == 0 and p["edge_blocks"] == 2, p
    p = plan(lib, big, vertex_program=1)
    assert p["n_waves"] > 0 and p["fused_tail"] == 0, p


def test_other_launches_keep_two(lib):
    """a region terminal (its kernel joins from an auxiliary stream after the vertex launch), the split form of the workgroup program
    (vertex_workspace = 2) and a partition (ghost columns, ownership masks) keep the two-launch iteration"""
    from gcs_admm_amd.partition import build_partition, strip_owner
    from test_gpu_configs import _region_row
    p = plan(lib, _region_row())
    assert p["n_term"] > 0 and p["fused_tail"] == 0, p
    p = plan(lib, lattice_boxes(3, 3), vertex_workspace=2)
    assert p["n_split"] > 0 and p["n_wg"] == 0 and p["fused_tail"] == 0, p
    lat = lattice_boxes(4, 6)
    assert plan(lib, lat)["fused_tail"] == 1
    part = build_partition(lat, strip_owner(lat, 2), 0, 2)
    assert part.num_incidences > int(part.graph.inc_ptr[-1])
    d, keep, _ = __import__("gcs_admm_amd.abi", fromlist=["graph_desc"]).graph_desc(
        part.graph, state_dtype=0, device=0, num_incidences=part.num_incidences)          # ghost columns alone
    assert lib.fused_plan_make(C.byref(d)) == 0 and lib.fused_plan_get(b"fused_tail") == 0
    d, keep, _ = __import__("gcs_admm_amd.abi", fromlist=["graph_desc"]).graph_desc(
        lat, state_dtype=0, device=0, edge_counted=np.ones(lat.num_edges, np.uint8))         # an ownership mask alone
    assert lib.fused_plan_make(C.byref(d)) == 0 and lib.fused_plan_get(b"fused_tail") == 0


def test_launch_lds_covers_the_tail(lib):
    """the launch asks for max(plan LDS, what the tail needs): on a graph whose only generic workgroup is small (degree 2, 4 facets)
    the request still holds red[4][5] and the flag"""
    p = plan(lib, path3())
    assert p["fused_tail"] == 1 and p["n_wg"] == 1
    assert p["tail_lds_bytes"] == (EDGE_BLOCK // 64 * 5 + 1) * 8
    assert p["launch_lds_bytes"] >= p["tail_lds_bytes"] and p["launch_lds_bytes"] >= p["wg_lds_bytes"], p
