"""The split form of the workgroup program (csrc/vertex_wg.h wg_solve_vertex<..., SPLIT>: the units of a vertex in a separate buffer,
the handle's device-memory workspace on the GPU) compiled for the host (tests/hostemu/wg_split_emu.cpp).  Without a GPU: the split form
equals the in-LDS form bit for bit (same layout, same arithmetic, same order) for n = 1, 2, 3, 6, 8, generic rows and BOX, with the
tasks of every region in ascending and in descending order; on hubs too large for LDS it matches the CPU oracle, warm and cold."""
import ctypes as C

import numpy as np
import pytest

from gcs_admm_amd import IPM_TOL
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import lattice_boxes
from hostemu_lib import emu_library
from solve_agreement import Agreement, NewtonParity, oracle_step


@pytest.fixture(scope="module")
def libs():
    return {False: emu_library("wgsplitemu").wg_split_emu_vertex_step, True: emu_library("wgsplitemu_rev").wg_split_emu_vertex_step_rev}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Warm:
    """a zeroed warm-start workspace: one record per vertex, warm_start.h's layout (as test_hostemu_wg.py spells it out)"""

    def __init__(self, g):
        n, NW = g.n, 2 * g.n + 1
        deg, m = np.diff(g.inc_ptr), np.diff(g.poly_ptr)
        units = (4 + 2 * n + 2 * NW + 1) & ~1
        size = [units + (deg[v] + 1) * (2 * NW + 2 + 2 * m[v]) for v in range(g.num_vertices)]
        self.ptr = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
        self.buf = np.zeros(int(self.ptr[-1]))


def step(fn, g, zedge, mu, split, box=False, warm=None):
    c, NI, V = g.c, 2 * g.num_edges, g.num_vertices
    copy = np.zeros((c, NI)); xv = np.zeros((V, 2 * g.n)); zv = np.zeros_like(xv); yv = np.zeros(V)
    cnt = np.zeros(2, dtype=np.int32); st = np.zeros(V, dtype=np.int32); it = np.zeros(V, dtype=np.int32)
    r = fn(int(split), int(box), g.n, V, g.num_edges, NI, _p(g.inc_ptr), _p(g.inc_edge), _p(g.inc_out), _p(g.poly_ptr), _p(g.poly_A),
           _p(g.poly_b), _p(g.interior), g.src, g.dst, _p(zedge), _p(mu), C.c_double(IPM_TOL), 60,
           _p(warm.buf) if warm else None, _p(warm.ptr) if warm else None, _p(copy), _p(xv), _p(zv), _p(yv), _p(cnt), _p(st), _p(it))
    assert r == 0
    return copy, xv, zv, yv, cnt, st, it


CASES = [("n=1 chain", 1, False), ("n=2 benchmark4", 2, False), ("n=3", 3, False), ("n=3 box", 3, True), ("n=6", 6, False),
         ("n=6 box", 6, True), ("n=8", 8, False)]


def _graph(name, n):
    if name == "n=1 chain":
        from conftest import interval_chain
        from gcs_admm_amd.graph import graph_from_sets
        return graph_from_sets(*interval_chain(6))
    if name == "n=2 benchmark4":
        return load_fixture("benchmark4")[1]
    return lattice_boxes(4, 3, n=n, seed=1)


@pytest.mark.parametrize("name,n,box", CASES, ids=[c[0] for c in CASES])
def test_split_form_is_bitwise_the_in_lds_form(libs, oracle_lib, name, n, box):
    g = _graph(name, n)
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL)
    warms = {(s, r): Warm(g) for s in (0, 1) for r in (False, True)}      # each build restarts from its own records
    for it in range(4):
        z0, m0 = o.zedge.copy(), o.mu.copy()
        res = {(s, r): step(libs[r], g, z0, m0, s, box, warms[s, r]) for s in (0, 1) for r in (False, True)}
        for r in (False, True):
            a, b = res[0, r], res[1, r]
            for x, y in zip(a, b):
                assert np.array_equal(x, y)       # the split form: same bits as the in-LDS form, in either task order
            assert np.array_equal(warms[0, r].buf, warms[1, r].buf)
        assert (res[1, False][5] == 0).all() and np.isfinite(res[1, False][0]).all()
        # and the task order changes the reductions' summation order only
        assert np.abs(res[1, False][0] - res[1, True][0]).max() <= 1e-9
        assert o.vertex_step(1.0, 1.0) == 0
        o.edge_step(1.0)


def _star(k):
    from conftest import star_case
    from gcs_admm_amd.graph import graph_from_sets
    As, bs, n = star_case(k)
    return graph_from_sets(As, bs, n)


def _hub(n, spokes, generic=False):
    from test_gpu_vertex_workspace import hub_case
    return hub_case(n, spokes, generic=generic)


HUBS = [("n=2 degree 120", lambda: _star(60)), ("n=6 generic degree 30", lambda: _hub(6, 15, True)), ("n=8 degree 16", lambda: _hub(8, 8))]


@pytest.mark.parametrize("cold", [False, True], ids=["warm", "cold"])
@pytest.mark.parametrize("name,mk", HUBS, ids=[c[0] for c in HUBS])
def test_oversized_hub_matches_oracle(libs, oracle_lib, name, mk, cold):
    """the hubs gcsadmm_create refuses with vertex_workspace 0: the split form's vertex steps along an oracle run, every solve and its
    Newton iterations against the oracle's (tests/solve_agreement.py; a hub and its spokes are few generic vertices: 16 steps)"""
    g = mk()
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL, warm_start=not cold)
    warm = None if cold else Warm(g)
    diffs = []
    mode = "cold" if cold else "warm"
    agree, newton = Agreement(f"{name} {mode}"), NewtonParity(f"{name} {mode}")
    for it in range(16):
        a = step(libs[False], g, o.zedge.copy(), o.mu.copy(), 1, False, warm)
        fails, iters, per_vertex = oracle_step(o)
        assert fails == 0
        assert a[4][0] == 0
        gen = a[6] > 0
        mask = np.zeros(2 * g.num_edges, bool)
        for v in np.nonzero(gen)[0]:
            mask[g.inc_ptr[v]:g.inc_ptr[v + 1]] = True
        diffs.append(np.abs(a[0][:, mask] - o.copy[:, mask]).max())
        assert np.abs(a[3][gen] - o.yv[gen]).max() <= 5e-4
        agree.add(g, gen, a[0], a[3], o.copy, o.yv)
        newton.add(a[4][1], iters, a[4][0], fails, a[6][gen], per_vertex[gen])
        o.edge_step(1.0)
    diffs = np.array(diffs)
    assert diffs.max() <= 2e-3 and np.median(diffs) <= 1e-5, diffs
    agree.check()
    newton.check(cold)
