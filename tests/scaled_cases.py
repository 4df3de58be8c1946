"""Cases and the penalty schedule of the scaled vertex-step tests (test_scaled_steps.py: the host builds; test_gpu_scaled_steps.py:
the device), and the three judgements every such run gets.

Every vertex-step program reads its inputs through consensus_target (csrc/step_args.h: zedge - mu_scale * mu), takes rho into its
Newton system and into the warm-start rule (csrc/warm_start.h: a record is comparable only if it was left at the same rho, and
dT = rho * max |T - T_record|).  At rho = 1, mu_scale = 1 all of that is the identity, so the runs here follow the loop's own pattern
of penalty changes with tau_incr = 3, tau_decr = 2 (steps counted from 0):

  * rho starts at 1;
  * it is multiplied by 3 before steps 4 and 9, with mu_scale = 1 / 3 for that step only;
  * it is multiplied by 1 / 2 before steps 13 and 17, with mu_scale = 3 for that step only (the decrease branch rescales the duals by
    tau_incr, as the reference does: loop_reference.control_reference);
  * mu_scale = 1 on every other step; 22 steps.

So rho runs 1, 3, 9, 4.5, 2.25: none but the first a power of two, and both directions of a change are crossed from valid records.
Each step copies the oracle's state to the side under test, then calls oracle_step(o, rho, mu_scale) and o.edge_step(mu_scale).
"""
import os
import sys

import numpy as np

from solve_agreement import Agreement, NewtonParity

TAU_INCR, TAU_DECR = 3.0, 2.0
STEPS = 22
INCREASE_BEFORE, DECREASE_BEFORE = (4, 9), (13, 17)


def schedule(steps=STEPS):
    """[(rho, mu_scale, change)] of every step.  change: what the control step that follows the step decides (+1 increase, -1
    decrease, 0 neither) -- it produces the next step's pair (solve_agreement.device_newton takes it)"""
    out, rho = [], 1.0
    for it in range(steps):
        mu_scale = 1.0
        if it in INCREASE_BEFORE:
            rho *= TAU_INCR; mu_scale = 1.0 / TAU_INCR
        elif it in DECREASE_BEFORE:
            rho *= 1.0 / TAU_DECR; mu_scale = TAU_INCR
        out.append([rho, mu_scale, 0])
    for it in range(steps - 1):
        out[it][2] = +1 if it + 1 in INCREASE_BEFORE else (-1 if it + 1 in DECREASE_BEFORE else 0)
    return [tuple(s) for s in out]


def constant(steps=12):
    """rho = 1, mu_scale = 1 throughout"""
    return [(1.0, 1.0, 0)] * steps


def pattern(name):
    return schedule() if name == "schedule" else constant()


def graph(name):
    """the graphs of the scaled tests by name: a fixture, "lattice 5x4", "lattice 14x11", "lattice n=3" / "lattice n=6" (4 x 3 boxes
    in R^n), "star 40", "intervals" (a chain of 8 in R^1), "region row", "region scene" """
    from gcs_admm_amd.cases import load_fixture
    from gcs_admm_amd.graph import graph_from_sets, lattice_boxes
    if name == "lattice 5x4":
        return lattice_boxes(5, 4, seed=1)
    if name == "lattice 14x11":
        return lattice_boxes(14, 11, seed=7)
    if name.startswith("lattice n="):
        return lattice_boxes(4, 3, n=int(name.split("=")[1]), seed=1)
    if name == "star 40":
        from conftest import star_case
        As, bs, n = star_case(40)
        return graph_from_sets(As, bs, n)
    if name == "intervals":
        from conftest import interval_chain
        return graph_from_sets(*interval_chain(8))
    if name == "region row":
        return region_row()
    if name == "region scene":
        return region_scene(1)
    return load_fixture(name)[1]


def region_row():
    """three boxes in a row, the outer two are the terminals: s = [0,1] x [0,1], t = [2,3] x [0,1], between them [0.8,2.2] x [0,1].
    Shortest path: leave s and enter t at the faces x = 1 and x = 2 -> length 1 (with point terminals at the box centres: 2)"""
    from gcs_admm_amd.graph import graph_from_sets
    A = np.vstack([np.eye(2), -np.eye(2)])
    box = lambda x0, x1, y0, y1: (A, np.array([x1, y1, -x0, -y0], float))
    As, bs = {}, {}
    As['s'], bs['s'] = box(0, 1, 0, 1); As['t'], bs['t'] = box(2, 3, 0, 1); As[0], bs[0] = box(0.8, 2.2, 0, 1)
    return graph_from_sets(As, bs, 2)


def region_scene(seed, half=0.35):
    """a 4 x 4 polygon scene (tools/scale_demo.py) whose terminals are boxes of half-width `half` about the points they were"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from scale_demo import polygon_scene
    from gcs_admm_amd.graph import graph_from_sets
    As, bs = polygon_scene(4, seed=seed, m=3 + seed % 4)
    A = np.vstack([np.eye(2), -np.eye(2)])
    for key in ('s', 't'):
        pt = 0.5 * (bs[key][:2] - bs[key][2:])
        As[key], bs[key] = A, np.hstack([pt + half, -pt + half])
    return graph_from_sets(As, bs, 2)


class Judgement:
    """a run judged three ways (add() once per step):
      * Agreement.check() over all solves (f32: the rule of solve_agreement.per_solve_diffs the run is held to);
      * NewtonParity.check_warm() over the run;
      * a second NewtonParity over only the steps whose rho differs from the previous step's, by check_cold(): no record is
        comparable there, so every solve on both sides must start cold."""

    def __init__(self, label, f32=False):
        self.label, self.f32 = label, f32
        self.agree = Agreement(label)
        self.newton = NewtonParity(label + " warm")
        self.changed = NewtonParity(label + " after a change of rho")
        self._rho = None

    def add(self, g, solves, rho, copy, yv, copy_ref, yv_ref, total, total_ref, fails=0, fails_ref=0, per_vertex=None,
            per_vertex_ref=None):
        self.agree.add(g, solves, copy, yv, copy_ref, yv_ref, f32=self.f32)
        self._count(rho, total, total_ref, fails, fails_ref, per_vertex, per_vertex_ref)

    def add_diffs(self, rho, diffs, per_vertex, per_vertex_ref):
        """a step whose per-solve differences and Newton counts the caller computed (one entry per solve)"""
        self.agree.add_diffs(diffs)
        self._count(rho, sum(per_vertex), sum(per_vertex_ref), 0, 0, per_vertex, per_vertex_ref)

    def _count(self, rho, total, total_ref, fails, fails_ref, per_vertex, per_vertex_ref):
        self.newton.add(total, total_ref, fails, fails_ref, per_vertex, per_vertex_ref)
        if self._rho is not None and rho != self._rho:
            self.changed.add(total, total_ref, fails, fails_ref, per_vertex, per_vertex_ref)
        self._rho = rho

    def summary(self):
        return "\n".join([self.agree.summary(), self.newton.summary()] + ([self.changed.summary()] if self.changed.tot else []))

    def rejections(self, near_frac=None, close_frac=None):
        """the judgements that reject the run: a list of (which, message), empty for a run that passes"""
        bad = []
        for which, check in (("agreement", lambda: self.agree.check(near_frac, close_frac)), ("newton warm", self.newton.check_warm),
                             ("newton after a change", self.changed.check_cold if self.changed.tot else (lambda: None))):
            try:
                check()
            except AssertionError as e:
                bad.append((which, str(e).splitlines()[0]))
        return bad

    def check(self, near_frac=None, close_frac=None):
        bad = self.rejections(near_frac, close_frac)
        assert not bad, f"{self.label}: {bad}\n{self.summary()}"
