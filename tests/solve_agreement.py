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


def per_solve_diffs(g, gen, copy, yv, copy_ref, yv_ref, f32=False):
    """worst difference of every generic vertex over its incidence columns and its yv, one entry per vertex in gen.  f32: the
    difference beyond one f32 ulp of the reference's word (zero for a word the device stored as the f32 nearest the oracle's)"""
    copy = np.asarray(copy, dtype=np.float64); copy_ref = np.asarray(copy_ref, dtype=np.float64)
    dc = np.abs(copy - copy_ref)
    dy = np.abs(np.asarray(yv, dtype=np.float64) - np.asarray(yv_ref, dtype=np.float64))
    if f32:
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


def device_newton(d, rho=1.0):
    """(Newton iterations, inner failures) of a DeviceSolver's vertex steps since its last control step: a control step moves the
    handle's counters into the control block.  Its sums give equal primal and dual residuals far above any stop threshold, so the
    penalty, the dual scale and the status stay as they were."""
    torch = d.torch
    sums = torch.tensor([1e4, 0.5e4 / rho ** 2, 0.0, 0.0, 0.0], dtype=torch.float64, device=d.device)
    d.control(sums)
    cb = d.read_control()
    assert cb.status == -1 and cb.rho == rho and cb.mu_scale == 1.0, (cb.status, cb.rho, cb.mu_scale)
    return cb.inner_iters, cb.inner_failures
