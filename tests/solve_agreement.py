"""Per-solve agreement of a vertex step with the CPU oracle, and Newton-iteration parity.

The legacy statistic of the vertex-step tests (worst coupled word of a step <= 2e-3, median over steps of that per-step worst
<= 1e-5) leaves four orders of magnitude between a typical solve (agrees with the oracle to ~1e-10) and the bound: a kernel can
be systematically wrong there and still pass.  The contract here judges every solve on its own:

  * per generic vertex and step, the worst difference over its incidence columns (every coupled word) and its yv;
  * pooled over the run: the worst of them within the legacy bound, a fraction NEAR_FRAC of the solves within NEAR and a fraction
    CLOSE_FRAC within CLOSE (f32 state: NEAR / CLOSE above one f32 ulp of the oracle's word, the oracle being given the same
    f32-rounded state);
  * Newton parity: no inner failure on either side; cold solves (oracle warm_start=False, device reset(cold_start=True), host
    builds without records) take per-step totals within COLD_STEP_DIFF and, where a side exposes them, the same iterations per
    vertex (a fraction COLD_VERTEX_EQUAL, the rest off by one); warm runs take run totals within WARM_TOTAL_REL + WARM_SLACK and,
    where exposed, the same per-vertex counts in a fraction WARM_VERTEX_EQUAL of the solves.

Measured with the host builds of the two device programs (tests/hostemu) against the oracle at IPM_TOL = 3e-9, 30 steps from
identical state on benchmark1, benchmark3, benchmark4, test_autogen2 and a 5 x 4 lattice, warm and cold, pooled over
(vertex, step): 0.80 - 0.98 of the solves within 1e-9, 0.94 - 0.997 within 1e-7, worst 6.5e-4 (a
step-length decision flipped by round-off late in a solve).  Seeded errors the legacy statistic passes and this contract
rejects (tests/test_solve_agreement_mutants.py, 12 steps of benchmark4 / benchmark1): REG_DELTA x 1.1 (0.06 / 0.13 within 1e-9),
centring r^3 -> r^3 (1 - 1e-3 r) (0.39 / 0.25), NT scaling eta x 1.01 (Newton totals +2.4 % / +7.4 % warm, +1.2 % / +2.0 % cold).
The MI355X scores what the host build of the same program scores (tests/test_gpu_parity.py states the device figures), so the
device tests use the same thresholds.

Under a schedule of penalties and with f32 state (tests/scaled_cases.py: 22 steps, rho = 1, 3, 9, 4.5, 2.25 with mu_scale = 1 / 3 or 3
on the step of each change; tests/test_scaled_steps.py the host builds, tests/test_gpu_scaled_steps.py the device).  A run is judged
three ways: check() over all solves, check_warm() over the run, and check_cold() over the steps whose rho differs from the previous
step's (no record is comparable there: both sides start cold).  Every threshold is one of those above; the host-build measurements
they were checked against, per case as near / close / worst, warm total - oracle's, after-change total - oracle's:
  f64, schedule      wavefront  benchmark4 0.952 / 0.988 / 7.8e-5, +0, +0    benchmark1 0.886 / 0.977 / 4.8e-5, +1, +0
                                lattice 5x4 (generic and box variant) 0.970 / 0.998 / 3.3e-7, +0, +0
                     workgroup  benchmark4 0.957 / 0.993 / 4.5e-5, -2, +0    benchmark1 0.920 / 0.966 / 4.8e-5, +1, +0
                                lattice 5x4 0.968 / 1.0 / 6.8e-8, +0, +0     lattice n=3 (generic / BOX) 0.958 / 0.955, 0.992, 1.5e-6, +0, +0
                                lattice n=6 (both) 0.932 / 0.992 / 1.5e-6, +0, +0      star 40 0.930 / 0.988 / 6.8e-6, +0, +0
                     terminal   region row 1.0 / 1.0 / 1.6e-12, +0, +0       region scene 1.0 / 1.0 / 4.0e-11, +0, +0
                     per-vertex counts: equal in 0.9886 - 1 of the solves of a run, in all of the steps after a change
  f32 "nearest"      wavefront  benchmark4 rho = 1: 0.957 / 0.994 / 2.3e-6, +0     schedule: 0.964 / 0.991 / 2.5e-6, +13, +0
                                lattice 14x11 (box variant) 1.0 / 1.0 / 4.8e-11, +0           0.999 / 1.0 / 7.7e-8, +0, +0
                     workgroup  benchmark3 0.958 / 0.979 / 5.1e-7, +0                          0.945 / 0.973 / 8.8e-6, +0, +0
                                lattice n=3 BOX 0.993 / 1.0 / 2.4e-9, +0                       0.970 / 0.992 / 8.3e-7, +0, +0
                                lattice n=6 BOX 0.986 / 1.0 / 2.7e-8, +0                       0.958 / 0.992 / 5.8e-7, +0, +0
                                benchmark4 0.966 / 0.996 / 1.5e-7, +0                          0.967 / 0.992 / 4.4e-6, +13, +0
                                intervals (n = 1) 0.990 / 0.990 / 4.5e-7, +0                   0.994 / 1.0 / 3.8e-9, +0, +0
                                star 40 1.0 / 1.0 / 9.0e-10, +0                                0.947 / 0.989 / 1.4e-4, -1, +0
  The lowest f32 case (0.945 / 0.973) is as far above NEAR_FRAC = 0.7 / CLOSE_FRAC = 0.9 as the f64 cases are, so f32 state under
  the "nearest" rule uses the f64 thresholds unchanged.  (The +13 is one warm / cold decision flipped in one step of benchmark4:
  within WARM_SLACK.)
Seeded errors that are the identity at rho = 1, mu_scale = 1 or with f64 state, on benchmark4 / the 5 x 4 lattice under the schedule
(workgroup build; the wavefront build's figures are within 0.005 and the same iterations):
  "stale" (a record counts as comparable whatever its rho): 0.430 / 0.620 within 1e-9, warm totals -11.5 % / -3.0 %, the steps after
  a change off by up to 116 / 40 iterations;  "dT_norho" (dT without the factor rho): 0.386 / 0.382, totals -4.6 % / -3.5 %;
  "unscaled word" (mu_scale skipped on word 0): worst word 1.17 / 0.32, per-vertex counts equal in 0.89 / 0.88;
  "truncating store" (f32 state, 12 steps of benchmark4 at rho = 1): 0.964 / 0.996 under the one-ulp rule f32=True, which passes it,
  0.613 / 0.927 under f32="nearest" (the clean build: 0.957 - 0.966).
MI355X (tests/test_gpu_scaled_steps.py prints every case): f64 under the schedule 0.909 (benchmark1) - 0.970 within 1e-9, 0.966 - 1.0
within 1e-7, worst 4.5e-5, warm totals -2 .. +1; f32 0.945 (benchmark3, schedule) - 1.0, 0.973 - 1.0, worst 1.4e-4 (star 40, schedule: the
host build's figure), warm totals -1 .. +0; every step after a change of rho takes exactly the oracle's total; region scene with its
terminals in the mask 0.932 / 0.990 / 1.1e-6.  Per case the device is within 0.025 of the host builds' near fraction (a few solves).

Rotated polytopes in R^3 .. R^8 (tests/rotated_cases.py: the 4 x 3 lattice turned by one orthogonal Q, cases (n, lattice seed, rotation
seed, cuts); tests/test_rotated_steps.py the workgroup host build, tests/test_gpu_rotated_steps.py the device): 12 steps at rho = 1, 144
solves a run.  Same thresholds.  (a) against the oracle on the same rotated graph, (b) cold against the rotated solves of the oracle on
the AXIS-ALIGNED lattice; near / close / worst, Newton total - oracle's, per-vertex counts equal (tasks ascending; descending within
0.007 / 0.035 of these):
  case                 (a) warm                               (a) cold                          (b) cold
  (3, 1, 3, 0)         0.944 / 0.944 / 3.9e-4, -5, 0.951      0.951 / 0.965 / 3.9e-4, +0, 1.0   0.944 / 0.965 / 4.0e-4, +0, 1.0
  (4, 1, 4, 0)         0.958 / 0.958 / 1.1e-5, +0, 1.0        0.944 / 0.958 / 2.7e-4, +0, 1.0   0.944 / 0.958 / 2.7e-4, +0, 1.0
  (5, 7, 605, 0)       0.931 / 0.951 / 2.8e-4, +2, 0.979      0.924 / 0.958 / 5.9e-4, +0, 1.0   0.924 / 0.958 / 2.0e-4, +1, 0.993
  (6, 2, 106, 0)       0.938 / 0.965 / 1.8e-4, +4, 0.986      0.944 / 0.958 / 2.1e-5, +0, 1.0   0.944 / 0.972 / 5.8e-5, +0, 1.0
  (7, 3, 207, 0)       0.944 / 0.979 / 5.4e-4, -1, 0.993      0.931 / 0.965 / 2.3e-4, +0, 1.0   0.931 / 0.972 / 1.9e-4, +0, 1.0
  (8, 4, 308, 0)       0.931 / 0.979 / 5.4e-4, +0, 1.0        0.944 / 0.979 / 4.4e-4, +0, 1.0   0.938 / 0.972 / 4.3e-4, +0, 1.0
  (3, 1, 3, 2)         0.938 / 0.951 / 7.3e-4, -9, 0.965      0.938 / 0.979 / 1.9e-5, +0, 1.0   0.944 / 0.979 / 7.0e-6, +0, 1.0
  (4, 1, 4, 3)         0.944 / 0.951 / 1.2e-4, +15, 0.951     0.944 / 0.993 / 1.1e-4, +0, 1.0   0.944 / 0.986 / 2.6e-7, +0, 1.0
  (6, 2, 106, 4)       0.944 / 0.979 / 1.1e-5, +2, 0.986      0.924 / 0.965 / 2.6e-6, +0, 1.0   0.931 / 0.972 / 2.0e-6, +0, 1.0
  (8, 4, 308, 5)       0.931 / 0.965 / 3.7e-6, +0, 1.0        0.924 / 0.972 / 7.2e-5, +0, 1.0   0.924 / 0.986 / 6.3e-7, +0, 1.0
The closest to a threshold: warm per-vertex counts equal in 0.951 of the solves on (3, 1, 3, 0) and (4, 1, 4, 3) against
WARM_VERTEX_EQUAL = 0.95 (seven solves of 144 one iteration apart: one warm / cold decision flipped).  No inner failure on either side
(before gcs_math::step_finite the cases at n = 5 .. 8 had them: test_rotated_steps.py quotes the census).  Seeded error that is the
identity on boxes -- ONE off-diagonal facet product of the K assembly (facet 0, entry (1, 0)) times 1 + 1e-3: bit for bit the clean build
on the lattices at n = 3, 6; on (3, 1, 3, 0) / (6, 2, 106, 0) 0.10 - 0.16 / 0.10 within 1e-9 under (a) and (b), 9 / 25 inner failures.
MI355X (tests/test_gpu_rotated_steps.py prints every case): (a) warm, cuts 0 at n = 3, 5, 6, 7, 8: 0.944 / 0.944 / 3.9e-4, +4;  0.931 / 0.958 /
4.4e-4, +0;  0.938 / 0.951 / 1.9e-4, +4;  0.944 / 0.979 / 5.6e-4, -1;  0.931 / 0.979 / 5.1e-4, +0;  (4, 1, 4, 3): 0.944 / 0.951 / 1.1e-4, +15;
(8, 4, 308, 5): 0.931 / 0.965 / 3.2e-6, +0.  (b) cold at n = 3, 6, 8: 0.944 / 0.972 / 3.8e-4;  0.944 / 0.965 / 4.8e-5;  0.938 / 0.972 / 3.1e-4, every
per-step total the oracle's.  n = 6 from the device-memory workspace 0.938 / 0.958 / 1.2e-4, +0; with f32 state ("nearest") 0.944 / 0.965 /
6.7e-5, +0.  The four seeds that failed before, cold and warm through step 8: no inner failure, totals -10 .. +0.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

# ---- the legacy statistic (kept beside the contract, unchanged)
WORST = 2e-3          # one coupled word of one step: a flipped step-length decision moves a weakest word by up to ~6e-4
LEGACY_MEDIAN = 1e-5  # median over steps of the per-step worst

# ---- per-solve agreement
NEAR, CLOSE = 1e-9, 1e-7
NEAR_FRAC = 0.7       # host builds: 0.80 - 0.98 within 1e-9 over 30 steps, lowest benchmark1 cold (four generic vertices, whose late
                      # sub-problems are nearly flat: 0.725 over 40 steps, on the MI355X too); REG_DELTA x 1.1 scores 0.06 - 0.13
CLOSE_FRAC = 0.9      # host builds: 0.94 - 0.997 within 1e-7 (benchmark1 cold over 40 steps: 0.92); the centring mutant scores 0.25 -
                      # 0.39 within 1e-9, REG_DELTA x 1.1 0.57 - 0.67 within 1e-7

# ---- Newton parity
COLD_STEP_DIFF = 1    # cold per-step totals, host builds: equal or off by one (one solve at the stop test's edge)
COLD_VERTEX_EQUAL = 0.99  # cold per-vertex counts, workgroup host build: equal in 0.9967 - 1 of the solves, never off by more than one
WARM_TOTAL_REL = 5e-3  # warm run totals: within WARM_TOTAL_REL of the oracle's plus WARM_SLACK iterations.  A count that differs by
WARM_SLACK = 24        # one at the stop test's edge can flip a later warm / cold decision of that vertex (warm_start.h), which moves
                       # a total by the ~10 - 12 iterations a cold solve costs over a warm one: two such flips are allowed.  Host
                       # builds on the fixtures: within 24 iterations (0.50 %: the wavefront build, benchmark4, 20 steps); on the
                       # random scenes of test_random_scenes_fuzz the workgroup build is off by 10, 22 and 10 iterations (one or two
                       # flips, up to 1.0 % of those short runs).  eta x 1.01: +2.4 % / +7.4 % warm (74 / 29 iterations)
WARM_VERTEX_EQUAL = 0.95  # warm per-vertex counts where a side exposes them: host builds 0.992 - 1 on the fixtures (eta x 1.01:
                          # 0.44 - 0.68)


def generic_mask(g):
    """the vertices that run the interior-point solve: not s, not t, at least one incoming and one outgoing edge"""
    deg = np.diff(g.inc_ptr)
    din = np.array([int((g.inc_out[g.inc_ptr[v]:g.inc_ptr[v + 1]] == 0).sum()) for v in range(g.num_vertices)])
    gen = (din > 0) & (deg - din > 0)
    gen[g.src] = False; gen[g.dst] = False
    return gen


def f32_round(a):
    """the state a device with f32 storage sees: what the oracle gets in an f32 comparison"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def nearest_excess(a, ref):
    """the f32 "nearest" rule: |a - ref| beyond HALF an f32 spacing taken at the larger magnitude of the two words.  A correctly
    rounded f32 store of a double within delta of ref has excess <= delta (the store moves it by at most half a spacing of its own
    binade, and the larger of the two magnitudes is in that binade or above); a store that rounds toward zero is off by up to a
    whole spacing, so half of one is left"""
    a = np.asarray(a, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    big = np.maximum(np.abs(a), np.abs(ref)).astype(np.float32)
    return np.maximum(np.abs(a - ref) - 0.5 * np.spacing(big).astype(np.float64), 0.0)


def per_solve_diffs(g, gen, copy, yv, copy_ref, yv_ref, f32=False):
    """worst difference of every generic vertex over its incidence columns and its yv, one entry per vertex in gen.  f32=True: the
    difference beyond one f32 ulp of the reference's word (zero for a word the device stored as the f32 nearest the oracle's).
    f32="nearest": the stricter rule of nearest_excess over the copy columns (y_v is kept in f64 on every side: plain difference)"""
    copy = np.asarray(copy, dtype=np.float64); copy_ref = np.asarray(copy_ref, dtype=np.float64)
    dc = np.abs(copy - copy_ref)
    dy = np.abs(np.asarray(yv, dtype=np.float64) - np.asarray(yv_ref, dtype=np.float64))
    if isinstance(f32, str):
        assert f32 == "nearest", f32
        dc = nearest_excess(copy, copy_ref)
    elif f32:
        dc = np.maximum(dc - np.spacing(np.abs(copy_ref).astype(np.float32)).astype(np.float64), 0.0)
        dy = np.maximum(dy - np.spacing(np.abs(np.asarray(yv_ref)).astype(np.float32)).astype(np.float64), 0.0)
    col = np.nan_to_num(dc, nan=np.inf).max(axis=0)
    vs = np.nonzero(gen)[0]
    out = np.empty(len(vs))
    for i, v in enumerate(vs):
        lo, hi = g.inc_ptr[v], g.inc_ptr[v + 1]
        out[i] = max(col[lo:hi].max() if hi > lo else 0.0, dy[v] if np.isfinite(dy[v]) else np.inf)
    return out


class Agreement:
    """per-solve differences pooled over a run (add() once per step), judged by check()"""

    def __init__(self, label=""):
        self.label = label
        self.steps = []

    def add(self, g, gen, copy, yv, copy_ref, yv_ref, f32=False):
        d = per_solve_diffs(g, gen, copy, yv, copy_ref, yv_ref, f32)
        self.steps.append(d)
        return d

    def add_diffs(self, d):
        """per-solve differences computed by the caller (one entry per solve)"""
        self.steps.append(np.atleast_1d(np.asarray(d, dtype=np.float64)))

    @property
    def pooled(self):
        return np.concatenate(self.steps) if self.steps else np.zeros(0)

    def stats(self):
        p = self.pooled
        return dict(solves=len(p), near=float((p <= NEAR).mean()), close=float((p <= CLOSE).mean()), worst=float(p.max()),
                    median=float(np.median(p)))

    def legacy_ok(self):
        """the statistic every vertex-step test used before: per-step worst <= 2e-3, median of per-step worsts <= 1e-5"""
        w = np.array([s.max() for s in self.steps])
        return bool(w.max() <= WORST and np.median(w) <= LEGACY_MEDIAN)

    def summary(self):
        p = self.pooled
        s = self.stats()
        q = np.quantile(p, [0.5, 0.9, 0.99]) if len(p) else [0, 0, 0]
        hist = {f"<=1e-{k}": float((p <= 10.0 ** -k).mean()) for k in (12, 10, 9, 8, 7, 6, 5, 4)}
        return (f"[agreement {self.label}] solves {s['solves']} within {NEAR:g}: {s['near']:.3f} within {CLOSE:g}: {s['close']:.3f} "
                f"worst {s['worst']:.2e} quantiles 50/90/99 % {q[0]:.1e}/{q[1]:.1e}/{q[2]:.1e} cumulative {hist}")

    def failures(self, near_frac=None, close_frac=None, worst=None):
        near_frac = NEAR_FRAC if near_frac is None else near_frac
        close_frac = CLOSE_FRAC if close_frac is None else close_frac
        worst = WORST if worst is None else worst
        s = self.stats()
        bad = []
        if not s["worst"] <= worst:
            bad.append(f"worst {s['worst']:.2e} > {worst:g}")
        if not s["near"] >= near_frac:
            bad.append(f"{s['near']:.3f} of solves within {NEAR:g} < {near_frac}")
        if not s["close"] >= close_frac:
            bad.append(f"{s['close']:.3f} of solves within {CLOSE:g} < {close_frac}")
        return bad

    def check(self, near_frac=None, close_frac=None, worst=None):
        print(self.summary())
        bad = self.failures(near_frac, close_frac, worst)
        assert not bad, "; ".join(bad) + "\n" + self.summary()


class NewtonParity:
    """Newton iterations of the two sides, step by step (add() once per step: totals, failures, per-vertex counts if exposed)"""

    def __init__(self, label=""):
        self.label = label
        self.tot, self.tot_ref, self.fails, self.fails_ref = [], [], [], []
        self.pv, self.pv_ref = [], []

    def add(self, total, total_ref, fails=0, fails_ref=0, per_vertex=None, per_vertex_ref=None):
        self.tot.append(int(total)); self.tot_ref.append(int(total_ref))
        self.fails.append(int(fails)); self.fails_ref.append(int(fails_ref))
        if per_vertex is not None and per_vertex_ref is not None:
            self.pv.append(np.asarray(per_vertex)); self.pv_ref.append(np.asarray(per_vertex_ref))

    def summary(self):
        t, r = np.array(self.tot), np.array(self.tot_ref)
        s = (f"[newton {self.label}] total {t.sum()} oracle {r.sum()} ({(t.sum() - r.sum()) / max(r.sum(), 1):+.4%}) "
             f"per-step |diff| max {np.abs(t - r).max() if len(t) else 0} failures {sum(self.fails)} / {sum(self.fails_ref)}")
        if self.pv:
            a, b = np.concatenate(self.pv), np.concatenate(self.pv_ref)
            s += f" per-vertex equal {(a == b).mean():.4f} of {len(a)}"
        return s

    def _no_failures(self):
        assert sum(self.fails) == 0 and sum(self.fails_ref) == 0, self.summary()

    def check_cold(self, step_diff=None):
        step_diff = COLD_STEP_DIFF if step_diff is None else step_diff
        print(self.summary())
        self._no_failures()
        d = np.abs(np.array(self.tot) - np.array(self.tot_ref))
        assert d.max() <= step_diff, f"cold per-step Newton totals differ by up to {d.max()} > {step_diff}\n" + self.summary()
        if self.pv:
            a, b = np.concatenate(self.pv), np.concatenate(self.pv_ref)
            assert np.abs(a - b).max() <= 1 and (a == b).mean() >= COLD_VERTEX_EQUAL, \
                "cold per-vertex Newton counts differ\n" + self.summary()

    def check_warm(self, rel=None, slack=None):
        rel = WARM_TOTAL_REL if rel is None else rel
        slack = WARM_SLACK if slack is None else slack
        print(self.summary())
        self._no_failures()
        a, b = sum(self.tot), sum(self.tot_ref)
        assert abs(a - b) <= rel * b + slack, \
            f"warm Newton run totals {a} / {b}: {a - b:+d} ({(a - b) / b:+.3%}) beyond {rel:.2%} + {slack}\n" + self.summary()
        if self.pv:
            eq = (np.concatenate(self.pv) == np.concatenate(self.pv_ref)).mean()
            assert eq >= WARM_VERTEX_EQUAL, f"warm per-vertex Newton counts equal in {eq:.3f} < {WARM_VERTEX_EQUAL}\n" + self.summary()

    def check(self, cold, **kw):
        self.check_cold(**kw) if cold else self.check_warm(**kw)


def oracle_step(o, rho=1.0, mu_scale=1.0):
    """one vertex step of the oracle with its per-vertex Newton counts: (failures, total iterations, per-vertex counts; a failed
    solve counts -(100 + its iterations), a special vertex 0)"""
    from oracle import oracle as O
    lib = O.lib()
    it = np.zeros(o.g.num_vertices, dtype=np.int32)
    before = o.ipm_iters.value
    lib.oracle_set_iters_out(it.ctypes.data_as(C.c_void_p))
    try:
        fails = o.vertex_step(rho, mu_scale)
    finally:
        lib.oracle_set_iters_out(None)
    return fails, o.ipm_iters.value - before, it


def device_newton(d, rho=1.0, change=0, tau_incr=2.0, tau_decr=2.0):
    """(Newton iterations, inner failures) of a DeviceSolver's vertex steps since its last control step: a control step moves the
    handle's counters into the control block.  change = 0: its sums give equal primal and dual residuals far above any stop
    threshold, so the penalty, the dual scale and the status stay as they were.  change = +1 / -1: the sums put pri / dual at 20 /
    at 1 / 20 under the current rho (nu = 10: far from the boundary either way; s2 .. s4 = 0, so no stop test fires), and the
    control step takes its increase / decrease branch -- rho x tau_incr with mu_scale 1 / tau_incr, or rho / tau_decr with mu_scale
    tau_incr (the reset's tau_incr, tau_decr: say them here) -- asserted bit for bit."""
    torch = d.torch
    pri2, dual2 = 1e4, 1e4                       # squares of the two residuals: pri = sqrt(s0), dual = rho sqrt(2 s1)
    if change > 0:
        dual2 = 1e4 / 400.0
    elif change < 0:
        pri2 = 1e4 / 400.0
    sums = torch.tensor([pri2, 0.5 * dual2 / rho ** 2, 0.0, 0.0, 0.0], dtype=torch.float64, device=d.device)
    d.control(sums)
    cb = d.read_control()
    want = (rho, 1.0) if change == 0 else ((rho * tau_incr, 1.0 / tau_incr) if change > 0 else (rho * (1.0 / tau_decr), tau_incr))
    assert cb.status == -1 and cb.rho == want[0] and cb.mu_scale == want[1], (cb.status, cb.rho, cb.mu_scale, want)
    return cb.inner_iters, cb.inner_failures
