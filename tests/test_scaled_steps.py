"""The host builds of the vertex-step programs (tests/hostemu: emu.cpp the wavefront program, wg_emu.cpp the workgroup program,
term_emu.cpp the region-terminal solve) against the oracle under the penalty schedule of tests/scaled_cases.py -- rho 1, 3, 9, 4.5,
2.25 with the dual scale 1 / 3 or 3 on the step of each change -- and with f32 state (the programs' float instantiations).  Every
run is judged three ways (scaled_cases.Judgement): per-solve agreement, the warm Newton total of the run, and the steps that follow
a change of rho as cold steps.  f32 runs are held to the "nearest" rule of solve_agreement.py.

Seeded errors that are the identity at rho = 1, mu_scale = 1 or with f64 state -- so nothing else in the suite sees them -- are
built through mutant_build and must be rejected (the figures: solve_agreement.py):
  * "stale": the warm-start rule forgets that a record is comparable only at the rho it was left at (vertex_wg.h, vertex_program.inc);
  * "dT_norho": dT = max |T - T_record| without the factor rho (both programs);
  * "unscaled word": consensus_target applies mu_scale to every word but word 0 (step_args.h);
  * "truncating store": the (T) stores of the copy columns round toward zero -- passes the one-ulp f32 rule, fails "nearest".
The device tests of the same cases are tests/test_gpu_scaled_steps.py."""
import ctypes as C
import os

import numpy as np
import pytest

from gcs_admm_amd import IPM_TOL
from mutant_build import build_mutants
from scaled_cases import Judgement, graph, pattern
from solve_agreement import f32_round, generic_mask, oracle_step
from hostemu_lib import emu_library
from test_hostemu import WarmRecords as WaveRecords
from test_hostemu_wg import WarmRecords as WgRecords

HERE = os.path.dirname(os.path.abspath(__file__))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.fixture(scope="module")
def wave():
    return emu_library("emu")


@pytest.fixture(scope="module")
def wg():
    return emu_library("wgemu")


@pytest.fixture(scope="module")
def term():
    return emu_library("termemu")


def _state_args(g, zedge, mu, rho, mu_scale, f32):
    """the arguments the two step functions share, and the outputs they fill"""
    dt = np.float32 if f32 else np.float64
    z, m = np.ascontiguousarray(zedge, dtype=dt), np.ascontiguousarray(mu, dtype=dt)
    c, NI, V = g.c, 2 * g.num_edges, g.num_vertices
    out = dict(copy=np.zeros((c, NI), dtype=dt), xv=np.zeros((V, 2 * g.n)), zv=np.zeros((V, 2 * g.n)), yv=np.zeros(V),
               cnt=np.zeros(2, dtype=np.int32), gen=np.zeros(V, dtype=np.int32))
    args = [g.n, V, g.num_edges, NI, _p(g.inc_ptr), _p(g.inc_edge), _p(g.inc_out), _p(g.poly_ptr), _p(g.poly_A), _p(g.poly_b),
            _p(g.interior), g.src, g.dst, _p(z), _p(m), C.c_double(rho), C.c_double(mu_scale), C.c_double(1e-4), C.c_double(IPM_TOL), 60,
            _p(out["copy"]), _p(out["xv"]), _p(out["zv"]), _p(out["yv"]), _p(out["cnt"]), _p(out["gen"])]
    return args, out, (z, m)


class WaveSide:
    """the wavefront program's host build: box = the canonical-box instantiation (what a lattice runs on the device)"""

    def __init__(self, lib, g, f32=False, box=False):
        self.lib, self.g, self.f32 = lib, g, f32
        self.fn = "emu_vertex_step_box" if box else "emu_vertex_step"
        self.warm = WaveRecords(g)

    def step(self, zedge, mu, rho, mu_scale):
        pv = np.zeros(self.g.num_vertices, dtype=np.int32)
        getattr(self.lib, self.fn + "_set_warm")(_p(self.warm.buf), _p(self.warm.ptr))
        getattr(self.lib, self.fn + "_set_iters")(_p(pv))
        args, out, keep = _state_args(self.g, zedge, mu, rho, mu_scale, self.f32)
        assert getattr(self.lib, self.fn + ("_f32" if self.f32 else ""))(*args) == 0
        gen = out["gen"] == 1
        assert pv[gen].sum() == out["cnt"][1]
        return out["copy"], out["yv"], int(out["cnt"][1]), int(out["cnt"][0]), gen, pv


class WgSide:
    """the workgroup program's host build: box = the BOX instantiation (n = 3, 6 lattices of canonical boxes on the device)"""

    def __init__(self, lib, g, f32=False, box=False):
        self.lib, self.g, self.f32, self.box = lib, g, f32, box
        self.warm = WgRecords(lib, g)

    def step(self, zedge, mu, rho, mu_scale):
        V = self.g.num_vertices
        st, it = np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32)
        self.lib.wg_emu_set_warm(_p(self.warm.buf), _p(self.warm.ptr))
        args, out, keep = _state_args(self.g, zedge, mu, rho, mu_scale, self.f32)
        self.lib.wg_emu_set_box(int(self.box))
        try:
            assert getattr(self.lib, "wg_emu_vertex_step_f32" if self.f32 else "wg_emu_vertex_step")(*args, _p(st), _p(it)) == 0
        finally:
            self.lib.wg_emu_set_box(0)
        return out["copy"], out["yv"], int(out["cnt"][1]), int(out["cnt"][0]), out["gen"] == 1, it


def run(oracle_lib, side, g, steps, label, f32=False):
    """the steps of a pattern (scaled_cases.schedule / constant) from the oracle's state; f32: both sides solve from the f32-rounded
    state, and the run is held to the "nearest" rule"""
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL)
    j = Judgement(label, f32="nearest" if f32 else False)
    for rho, mu_scale, _ in steps:
        if f32:
            o.zedge[...] = f32_round(o.zedge); o.mu[...] = f32_round(o.mu)
        copy, yv, total, fails, gen, pv = side.step(o.zedge.copy(), o.mu.copy(), rho, mu_scale)
        fails_ref, total_ref, pv_ref = oracle_step(o, rho, mu_scale)
        j.add(g, gen, rho, copy, yv, o.copy, o.yv, total, total_ref, fails, fails_ref, pv[gen], pv_ref[gen])
        o.edge_step(mu_scale)
    return j


# ---- the schedule, f64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,box", [("benchmark4", False), ("benchmark1", False), ("lattice 5x4", False), ("lattice 5x4", True)])
def test_wavefront_program_under_the_schedule(wave, oracle_lib, name, box):
    g = graph(name)
    j = run(oracle_lib, WaveSide(wave, g, box=box), g, pattern("schedule"), f"wavefront {name}{' box' if box else ''} schedule")
    j.check()


@pytest.mark.parametrize("name,box", [("benchmark4", False), ("benchmark1", False), ("lattice 5x4", False), ("lattice n=3", False),
                                      ("lattice n=3", True), ("lattice n=6", False), ("lattice n=6", True), ("star 40", False)])
def test_workgroup_program_under_the_schedule(wg, oracle_lib, name, box):
    g = graph(name)
    j = run(oracle_lib, WgSide(wg, g, box=box), g, pattern("schedule"), f"workgroup {name}{' box' if box else ''} schedule")
    j.check()


@pytest.mark.parametrize("name", ["region row", "region scene"])
def test_region_terminal_solve_under_the_schedule(term, oracle_lib, name):
    """terminal_region.h has its own rec[1] == P.rho test: the two terminals' solves along an oracle run under the schedule, each
    restarted from its own record, against the oracle's solve_terminal_region of the same step (the oracle's step over the whole
    graph: its columns and its Newton count of the terminal)"""
    from test_terminal_region import emu_terminal
    g = graph(name)
    n = g.n
    term.term_emu_record_doubles.restype = C.c_longlong
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL)
    j = Judgement(f"terminals of {name} schedule")
    recs = {}
    for v in (g.src, g.dst):
        lo, hi = int(g.inc_ptr[v]), int(g.inc_ptr[v + 1])
        d_in = int((g.inc_out[lo:hi] == 0).sum())
        assert (g.inc_out[lo:lo + d_in] == 0).all()                     # incoming incidences first, as the solve takes them
        live = hi - lo - d_in if v == g.src else d_in
        m = int(g.poly_ptr[v + 1] - g.poly_ptr[v])
        recs[v] = (lo, hi, d_in, np.zeros(term.term_emu_record_doubles(n, m, live)))
    for rho, mu_scale, _ in pattern("schedule"):
        z0, m0 = o.zedge.copy(), o.mu.copy()
        fails_ref, _, pv_ref = oracle_step(o, rho, mu_scale)
        assert fails_ref == 0
        diffs, its, its_ref = [], [], []
        for v, (lo, hi, d_in, rec) in recs.items():
            T = np.ascontiguousarray(z0[:, g.inc_edge[lo:hi]] - mu_scale * m0[:, lo:hi])
            p0, p1 = int(g.poly_ptr[v]), int(g.poly_ptr[v + 1])
            e = emu_terminal(term, n, np.ascontiguousarray(g.poly_A[p0:p1]), np.ascontiguousarray(g.poly_b[p0:p1]),
                             np.ascontiguousarray(g.interior[v]), hi - lo, d_in, v == g.src, T, rho, warm=rec)
            assert pv_ref[v] > 0                                        # the oracle ran its region solve, not the closed form of a point
            diffs.append(max(np.abs(e[0] - o.copy[:, lo:hi]).max(), np.abs(e[1] - o.xv[v]).max()))
            its.append(e[4]); its_ref.append(int(pv_ref[v]))
        j.add_diffs(rho, diffs, its, its_ref)
        o.edge_step(mu_scale)
    j.check()


# ---- f32 state ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", ["rho = 1", "schedule"])
@pytest.mark.parametrize("name,box", [("benchmark4", False), ("lattice 14x11", True)])
def test_wavefront_program_f32_state(wave, oracle_lib, name, box, steps):
    g = graph(name)
    j = run(oracle_lib, WaveSide(wave, g, f32=True, box=box), g, pattern(steps), f"wavefront f32 {name} {steps}", f32=True)
    j.check()


@pytest.mark.parametrize("steps", ["rho = 1", "schedule"])
@pytest.mark.parametrize("name,box", [("benchmark3", False), ("lattice n=3", True), ("lattice n=6", True),
                                      # the further f32 cases of the device tests, for the host build's score of each
                                      ("benchmark4", False), ("intervals", False), ("star 40", False)])
def test_workgroup_program_f32_state(wg, oracle_lib, name, box, steps):
    g = graph(name)
    j = run(oracle_lib, WgSide(wg, g, f32=True, box=box), g, pattern(steps), f"workgroup f32 {name} {steps}", f32=True)
    j.check()


# ---- seeded errors -----------------------------------------------------------------------------------------------------------------
TRUNC = ("([](double x) { float f = (float)x; if (fabs((double)f) > fabs(x)) f = nextafterf(f, 0.0f); return (double)f; })")
WG_MUTANTS = {
    "clean": [],
    "stale": [("wrec[0] == 1.0 && wrec[1] == rho", "wrec[0] == 1.0")],
    "dT_norho": [("comparable ? -rt.mn * rho : -1.0", "comparable ? -rt.mn : -1.0")],
    "truncating store": [("(T)val, a.publish", f"(T)(sizeof(T) == 4 ? {TRUNC}(val) : val), a.publish")],
}
WAVE_MUTANTS = {
    "clean": [],
    "stale": [("rec[0] == 1.0 && rec[1] == rho;", "rec[0] == 1.0;")],
    "dT_norho": [("comparable ? rho * fmax(", "comparable ? fmax(")],
    "truncating store": [("= (T)(L.out ? o1 : tfree);", f"= (T)(sizeof(T) == 4 ? {TRUNC}(L.out ? o1 : tfree) : (L.out ? o1 : tfree));"),
                         ("= (T)(L.out ? o2 : o1);", f"= (T)(sizeof(T) == 4 ? {TRUNC}(L.out ? o2 : o1) : (L.out ? o2 : o1));"),
                         ("= (T)L.yy;", f"= (T)(sizeof(T) == 4 ? {TRUNC}(L.yy) : L.yy);")],
}
ARGS_MUTANTS = {
    "unscaled word": [("- mu_scale * (double)a.mu[", "- (w == 0 ? 1.0 : mu_scale) * (double)a.mu[")],
}
RHO_MUTANTS = ["stale", "dT_norho"]
MUTANT_GRAPHS = ["benchmark4", "lattice 5x4"]


@pytest.fixture(scope="module")
def wg_mutants(tmp_path_factory):
    src = os.path.join(HERE, "hostemu", "wg_emu.cpp")
    libs = build_mutants(tmp_path_factory.mktemp("wg_mutants"), "vertex_wg.h", WG_MUTANTS, src)
    libs.update(build_mutants(tmp_path_factory.mktemp("args_mutants"), "step_args.h", ARGS_MUTANTS, src))
    return libs


@pytest.fixture(scope="module")
def wave_mutants(tmp_path_factory):
    return build_mutants(tmp_path_factory.mktemp("wave_mutants"), "vertex_program.inc", WAVE_MUTANTS, os.path.join(HERE, "hostemu", "emu.cpp"))


@pytest.mark.parametrize("name", MUTANT_GRAPHS)
def test_clean_copies_pass_the_schedule(wg_mutants, wave_mutants, oracle_lib, name):
    g = graph(name)
    for side in (WgSide(wg_mutants["clean"], g), WaveSide(wave_mutants["clean"], g)):
        j = run(oracle_lib, side, g, pattern("schedule"), f"clean {type(side).__name__} {name}")
        print(j.summary())
        j.check()


@pytest.mark.parametrize("name", MUTANT_GRAPHS)
@pytest.mark.parametrize("mutant", RHO_MUTANTS + ["unscaled word"])
def test_workgroup_program_seeded_errors_are_rejected(wg_mutants, oracle_lib, mutant, name):
    g = graph(name)
    j = run(oracle_lib, WgSide(wg_mutants[mutant], g), g, pattern("schedule"), f"workgroup {mutant} {name}")
    bad = j.rejections()
    print(bad)
    assert bad, f"no judgement rejects the seeded error {mutant!r}:\n{j.summary()}"


@pytest.mark.parametrize("name", MUTANT_GRAPHS)
@pytest.mark.parametrize("mutant", RHO_MUTANTS)
def test_wavefront_program_seeded_errors_are_rejected(wave_mutants, oracle_lib, mutant, name):
    g = graph(name)
    j = run(oracle_lib, WaveSide(wave_mutants[mutant], g), g, pattern("schedule"), f"wavefront {mutant} {name}")
    bad = j.rejections()
    print(bad)
    assert bad, f"no judgement rejects the seeded error {mutant!r}:\n{j.summary()}"


@pytest.mark.parametrize("program", ["workgroup", "wavefront"])
def test_a_truncating_store_passes_the_one_ulp_rule_and_fails_nearest(wg_mutants, wave_mutants, oracle_lib, program):
    """f32 state whose (T) stores round toward zero: every word is within one f32 ulp of the oracle's, so the rule f32=True forgives
    it; beyond half a spacing about half of an ulp is left, ~1e-8 on words of order 0.1 - 1, and few solves stay within 1e-9"""
    g = graph("benchmark4")
    make = (lambda lib: WgSide(lib, g, f32=True)) if program == "workgroup" else (lambda lib: WaveSide(lib, g, f32=True))
    libs = wg_mutants if program == "workgroup" else wave_mutants
    clean = run(oracle_lib, make(libs["clean"]), g, pattern("rho = 1"), f"{program} f32 clean", f32=True)
    clean.check()
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL)
    side = make(libs["truncating store"])
    old, new = Judgement(f"{program} truncating store, one-ulp rule", f32=True), Judgement(f"{program} truncating store, nearest", f32="nearest")
    for rho, mu_scale, _ in pattern("rho = 1"):
        o.zedge[...] = f32_round(o.zedge); o.mu[...] = f32_round(o.mu)
        copy, yv, total, fails, gen, pv = side.step(o.zedge.copy(), o.mu.copy(), rho, mu_scale)
        fails_ref, total_ref, pv_ref = oracle_step(o, rho, mu_scale)
        for j in (old, new):
            j.add(g, gen, rho, copy, yv, o.copy, o.yv, total, total_ref, fails, fails_ref, pv[gen], pv_ref[gen])
        o.edge_step(mu_scale)
    print(old.summary()); print(new.summary())
    old.check()
    assert [which for which, _ in new.rejections()] == ["agreement"], new.summary()


def test_generic_mask_is_the_host_builds(wg, oracle_lib):
    """the device tests take generic_mask(g) where the host builds report their own: the same vertices"""
    for name in ("benchmark4", "lattice n=3"):
        g = graph(name)
        out = WgSide(wg, g).step(np.zeros((g.c, g.num_edges)), np.zeros((g.c, 2 * g.num_edges)), 1.0, 1.0)
        assert np.array_equal(out[4], generic_mask(g))
