"""The non-vertex half of an ADMM iteration restated in plain numpy, and the contract the device kernels are held to.

edge step (z-update, dual update, five norms: admm_solver_v3.py:543-614), loop control (residuals, rho adaptation, mu rescale,
stop test, trace record: admm_solver_v3.py:697-733) and the cost of the last iterate (GCS_utils.py:184-211), in this
repository's array layout: ``copy`` / ``mu`` are [c, NI], ``zedge`` is [c, E], c = 2n + 1 coupled words per copy, column
``tail[e]`` / ``head[e]`` of edge e.  No oracle, no torch: tests/test_loop_reference.py holds this file and the C oracle against
each other on the CPU, tests/test_gpu_edge_control.py holds edge_kernel (every launch mode), finalize_kernel, control_body and
cost_kernel of csrc/loop_kernels.h to it.

The bounds are derived, none is fitted to the code under test:

  zedge_new   bitwise.  0.5 * (a + b) in double is one rounding; for f32 state the double sum of two floats is exact and the
              result is rounded to f32 once, as the kernel does.
  mu_new      f64: bitwise when mu_scale is a power of two (the product is exact, one rounding left).  Otherwise the compiler may
              contract mu_scale * mu + r into an fma: per word |dev - ref| <= 2^-53 (|mu_scale mu| + |mu_new|).
              f32: the double value is rounded to f32 a second time, so a contracted product can move the result by one f32 ulp
              at most; the share of such words is reported, not bounded.
  five sums   every term is a square times a 0/1 weight, so ANY summation order is within (N - 1) 2^-53 relative of the exact
              sum of N terms; forming a term (a difference, a square, a possible fma) costs at most 4 more roundings.
              rtol = (N + 8) 2^-53, N = 2 E c for sums 0, 2, 4 and E c for sums 1, 3; an exactly zero sum must come out zero.
              The reference sum is taken in extended precision (numpy longdouble with a 64-bit mantissa, else math.fsum) from the
              ROUNDED zedge_new / mu_new, which is what the kernel squares.
  control     rho, mu_scale, it, status, inner_failures and the recorded sums exact; pri, dual, eps_pri, eps_dual and the trace
              row within 4 ulp (two roundings that contraction may merge, a device sqrt within an ulp).  The branches (>=, <)
              are taken by the reference on the DEVICE's pri / dual / eps (``decide_on``), so an ulp cannot flip a branch in a
              test; the boundary cases of CONTROL_TABLE are built from exactly representable values.
  cost        (V (n + 2) + E + 8) 2^-53 times the sum of the ABSOLUTE terms (an edge activation may be slightly negative).
"""
from __future__ import annotations

import math

import numpy as np

RUNNING, CONVERGED, MAX_IT, DIVERGED = -1, 0, 1, 2
EPS53 = 2.0 ** -53
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63
ULPS = 4                      # pri, dual, eps_pri, eps_dual, trace row
SUM_NAMES = ("|r|^2", "|dz|^2", "|copy|^2", "|zedge|^2", "|mu|^2")
CB_EXACT = ("rho", "mu_scale", "it", "status", "inner_failures")
CB_ULP = ("pri", "dual", "eps_pri", "eps_dual")


def _wide(a):
    return np.asarray(a, dtype=np.float64).astype(np.longdouble) if LONGDOUBLE_OK else np.asarray(a, dtype=np.float64)


def _total(terms) -> float:
    """sum of the terms, rounded to double once (longdouble: 2^-64 per addition, far inside every bound below; else exact)"""
    if LONGDOUBLE_OK:
        return float(np.sum(terms, dtype=np.longdouble))
    return math.fsum(np.asarray(terms, dtype=np.float64).ravel().tolist())


# -------------------------------------------------------------------------------------------------
# edge step
# -------------------------------------------------------------------------------------------------
def edge_reference(tail, head, copy, zedge_old, mu_old, mu_scale, inc_counted=None, edge_counted=None, dtype=np.float64):
    """z-update, dual update and the five sums of one edge step.  Returns dict(zedge, mu, sums[5] float64, terms[5] int).

    Every edge updates both its columns, ghost columns included; the 0/1 weights ``inc_counted`` [NI] / ``edge_counted`` [E]
    (ownership rule of a vertex partition) only enter the sums."""
    dtype = np.dtype(dtype)
    tail = np.asarray(tail, dtype=np.int64); head = np.asarray(head, dtype=np.int64)
    copy = np.asarray(copy); zedge_old = np.asarray(zedge_old); mu_old = np.asarray(mu_old)
    assert copy.dtype == dtype and zedge_old.dtype == dtype and mu_old.dtype == dtype
    c, E = zedge_old.shape
    assert copy.shape == mu_old.shape and copy.shape[0] == c and tail.shape == head.shape == (E,)
    cu = copy[:, tail].astype(np.float64); cw = copy[:, head].astype(np.float64)
    zedge = (0.5 * (cu + cw)).astype(dtype)
    zn = zedge.astype(np.float64)
    ru = cu - zn; rw = cw - zn
    ms = np.float64(mu_scale)
    mu = mu_old.copy()
    mu[:, tail] = (ms * mu_old[:, tail].astype(np.float64) + ru).astype(dtype)
    mu[:, head] = (ms * mu_old[:, head].astype(np.float64) + rw).astype(dtype)
    wt = np.ones(E) if inc_counted is None else np.asarray(inc_counted)[tail].astype(np.float64)
    wh = np.ones(E) if inc_counted is None else np.asarray(inc_counted)[head].astype(np.float64)
    we = np.ones(E) if edge_counted is None else np.asarray(edge_counted).astype(np.float64)
    W = _wide
    Cu, Cw, Zn, Zo = W(cu), W(cw), W(zn), W(zedge_old)
    Mu, Mw = W(mu[:, tail]), W(mu[:, head])
    wt, wh, we = W(wt)[None, :], W(wh)[None, :], W(we)[None, :]
    Ru, Rw, Dz = Cu - Zn, Cw - Zn, Zn - Zo
    sums = np.array([_total(wt * Ru * Ru + wh * Rw * Rw), _total(we * Dz * Dz), _total(wt * Cu * Cu + wh * Cw * Cw),
                     _total(we * Zn * Zn), _total(wt * Mu * Mu + wh * Mw * Mw)], dtype=np.float64)
    return dict(zedge=zedge, mu=mu, sums=sums, terms=np.array([2 * E * c, E * c, 2 * E * c, E * c, 2 * E * c], dtype=np.int64),
                mu_scale=float(mu_scale), tail=tail, head=head, mu_old=mu_old)


def sum_rtol(terms) -> np.ndarray:
    return (np.asarray(terms, dtype=np.float64) + 8.0) * EPS53


def _is_pow2(x: float) -> bool:
    m, _ = math.frexp(abs(x))
    return x != 0 and m == 0.5


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def check_edge_step(case, ref, zedge, mu, sums):
    """Hold a device edge step (``zedge``, ``mu`` in the state type, ``sums`` [5] float64) to ``ref`` = edge_reference(...).
    Raises AssertionError naming the case, the word / edge / sum and both values.  Returns the figures a report wants:
    dict(sum_err_over_bound [5], worst_sum, mu_bitwise, mu_off_share)."""
    zedge = np.asarray(zedge); mu = np.asarray(mu); sums = np.asarray(sums, dtype=np.float64)
    assert zedge.dtype == ref["zedge"].dtype and mu.dtype == ref["mu"].dtype, f"{case}: state type"
    assert zedge.shape == ref["zedge"].shape and mu.shape == ref["mu"].shape and sums.shape == (5,), f"{case}: shapes"
    bad = _bits(zedge) != _bits(ref["zedge"])
    if bad.any():
        w, e = _first(bad)
        raise AssertionError(f"{case}: zedge word {w} edge {e} (columns {ref['tail'][e]}, {ref['head'][e]}): device {zedge[w, e]!r}, "
                             f"reference {ref['zedge'][w, e]!r} ({int(bad.sum())} of {bad.size} words differ)")
    diff = _bits(mu) != _bits(ref["mu"])
    off_share = float(diff.mean())
    if diff.any():
        m64, r64 = mu.astype(np.float64), ref["mu"].astype(np.float64)
        if mu.dtype == np.float64:
            if _is_pow2(ref["mu_scale"]):
                tol = np.zeros_like(r64)                                    # one rounding on either side: bitwise
            else:
                tol = EPS53 * (np.abs(ref["mu_scale"] * ref["mu_old"].astype(np.float64)) + np.abs(r64))
        else:
            tol = np.spacing(np.abs(ref["mu"])).astype(np.float64)          # one f32 ulp of mu_new
        with np.errstate(invalid="ignore"):
            bad = ~(np.abs(m64 - r64) <= tol) & diff
        if bad.any():
            w, k = _first(bad)
            edges = np.nonzero((ref["tail"] == k) | (ref["head"] == k))[0]
            raise AssertionError(f"{case}: mu word {w} column {k} (edge {edges.tolist()}): device {mu[w, k]!r}, reference {ref['mu'][w, k]!r}, "
                                 f"allowed {tol[w, k]:.3e} at mu_scale {ref['mu_scale']!r} ({int(bad.sum())} of {bad.size} words outside)")
    rtol = sum_rtol(ref["terms"])
    err = np.zeros(5)
    for k in range(5):
        r, d = float(ref["sums"][k]), float(sums[k])
        if r == 0.0:
            ok = d == 0.0
        else:
            err[k] = abs(d - r) / (rtol[k] * abs(r)) if np.isfinite(d) else np.inf
            ok = err[k] <= 1.0
        if not ok:
            raise AssertionError(f"{case}: sum {k} ({SUM_NAMES[k]}): device {d!r}, reference {r!r}, relative difference "
                                 f"{abs(d - r) / abs(r) if r else float('inf'):.3e}, bound {rtol[k]:.3e} ({int(ref['terms'][k])} terms)")
    return dict(sum_err_over_bound=err, worst_sum=float(err.max()), mu_bitwise=not diff.any(), mu_off_share=off_share)


# -------------------------------------------------------------------------------------------------
# loop control
# -------------------------------------------------------------------------------------------------
def control_block(rho=1.0, mu_scale=1.0, it=1, status=RUNNING, inner_failures=0, sums=(0.0,) * 5, pri=0.0, dual=0.0,
                  eps_pri=0.0, eps_dual=0.0):
    """the control block after a reset, as a dict (the fields of gcsadmm_control_block this contract covers)"""
    return dict(rho=float(rho), mu_scale=float(mu_scale), it=int(it), status=int(status), inner_failures=int(inner_failures),
                sums=np.array(sums, dtype=np.float64), pri=float(pri), dual=float(dual), eps_pri=float(eps_pri), eps_dual=float(eps_dual))


def control_params(tau_incr=2.0, tau_decr=2.0, nu=10.0, it_rho_limit=100, max_it=1000, eps_abs=1e-4, eps_rel=1e-3, rho=1.0):
    return dict(tau_incr=float(tau_incr), tau_decr=float(tau_decr), nu=float(nu), it_rho_limit=int(it_rho_limit), max_it=int(max_it),
                eps_abs=float(eps_abs), eps_rel=float(eps_rel), rho=float(rho))


def control_reference(cb, sums, params, nx, nmu, fails, decide_on=None):
    """One control step on the five (globally reduced) sums.  Returns (new control block, trace row [6] or None, trace index).

    A block whose status has left RUNNING does not change.  Non-finite total: DIVERGED with rho, mu_scale, it, the residuals and
    the trace untouched (the sums and the failure count of the step are still recorded).  The decrease branch rescales mu by
    ``tau_incr``, not ``tau_decr``, as admm_solver_v3.py:708 does.  ``decide_on``: dict(pri, dual, eps_pri, eps_dual) whose values
    replace the reference's own in the comparisons (the device's, see the module docstring)."""
    p = params
    out = dict(cb); out["sums"] = np.array(cb["sums"], dtype=np.float64)
    if cb["status"] != RUNNING:
        return out, None, None
    s = np.array(sums, dtype=np.float64)[:5]
    out["sums"] = s.copy(); out["inner_failures"] = int(fails)
    with np.errstate(all="ignore"):
        tot = s[0] + s[1] + s[2] + s[3] + s[4]
        if not np.isfinite(tot):
            out["status"] = DIVERGED
            return out, None, None
        it, rho = int(cb["it"]), float(cb["rho"])
        pri = float(np.sqrt(s[0])); dual = float(rho * np.sqrt(2.0 * s[1]))
        dp, dd = (pri, dual) if decide_on is None else (decide_on["pri"], decide_on["dual"])
        mu_scale = 1.0
        if dp >= p["nu"] * dd and it < p["it_rho_limit"]:
            rho *= p["tau_incr"]; mu_scale = 1.0 / p["tau_incr"]
        elif dd >= p["nu"] * dp and it < p["it_rho_limit"]:
            rho *= 1.0 / p["tau_decr"]; mu_scale = p["tau_incr"]
        eps_pri = float(np.sqrt(nx) * p["eps_abs"] + p["eps_rel"] * max(np.sqrt(s[2]), np.sqrt(2.0 * s[3])))
        eps_dual = float(np.sqrt(nmu) * p["eps_abs"] + p["eps_rel"] * mu_scale * np.sqrt(s[4]))
    out.update(rho=rho, mu_scale=mu_scale, pri=pri, dual=dual, eps_pri=eps_pri, eps_dual=eps_dual)
    row = np.array([rho, pri, dual, eps_pri, eps_dual, float(fails)])
    ep, ed = (eps_pri, eps_dual) if decide_on is None else (decide_on["eps_pri"], decide_on["eps_dual"])
    if dp < ep and dd < ed:
        out["status"] = CONVERGED
        return out, row, it - 1
    out["it"] = it + 1
    if it + 1 > p["max_it"]:
        out["status"] = MAX_IT
    return out, row, it - 1


def cb_dict(cb):
    """a ctypes control block (gcs_admm_amd.solver.ControlBlock) as the dict control_reference works on"""
    return control_block(cb.rho, cb.mu_scale, cb.it, cb.status, cb.inner_failures, list(cb.sums), cb.pri, cb.dual, cb.eps_pri, cb.eps_dual)


def _same_double(a, b):
    return np.array_equal(_bits(np.array([a], dtype=np.float64)), _bits(np.array([b], dtype=np.float64)))


def _within_ulps(a, b, ulps=ULPS):
    a, b = float(a), float(b)
    if _same_double(a, b) or (np.isnan(a) and np.isnan(b)):
        return True
    if not (np.isfinite(a) and np.isfinite(b)):
        return False
    return abs(a - b) <= ulps * float(np.spacing(max(abs(a), abs(b))))


def check_control(case, ref, ref_row, ref_index, dev, trace_before=None, trace_after=None):
    """Hold the device's control block after a control step (``dev``: dict as cb_dict) and its trace (before / after, [max_it, 6])
    to control_reference's (``ref``, ``ref_row``, ``ref_index``).  Raises AssertionError naming case, field and both values."""
    for f in CB_EXACT:
        same = _same_double(ref[f], dev[f]) if f in ("rho", "mu_scale") else ref[f] == dev[f]
        if not same:
            raise AssertionError(f"{case}: control field {f}: device {dev[f]!r}, reference {ref[f]!r}")
    bad = _bits(np.asarray(dev["sums"], dtype=np.float64)) != _bits(np.asarray(ref["sums"], dtype=np.float64))
    if bad.any():
        k = _first(bad)[0]
        raise AssertionError(f"{case}: recorded sum {k} ({SUM_NAMES[k]}): device {dev['sums'][k]!r}, reference {ref['sums'][k]!r}")
    for f in CB_ULP:
        if not _within_ulps(ref[f], dev[f]):
            raise AssertionError(f"{case}: control field {f}: device {dev[f]!r}, reference {ref[f]!r} (more than {ULPS} ulp)")
    if trace_after is None:
        return
    before, after = np.asarray(trace_before, dtype=np.float64), np.asarray(trace_after, dtype=np.float64)
    changed = np.nonzero((_bits(before) != _bits(after)).any(axis=1))[0]
    if ref_row is None:
        if len(changed):
            raise AssertionError(f"{case}: trace row {int(changed[0])} was written by a step that records nothing: {after[changed[0]]!r}")
        return
    other = [int(r) for r in changed if r != ref_index]
    if other:
        raise AssertionError(f"{case}: trace row {other[0]} changed, the step records row {ref_index}: {after[other[0]]!r}")
    row = after[ref_index]
    for k, name in enumerate(("rho", "pri", "dual", "eps_pri", "eps_dual", "inner_failures")):
        ok = _same_double(row[k], ref_row[k]) if k in (0, 5) else _within_ulps(row[k], ref_row[k])
        if not ok:
            raise AssertionError(f"{case}: trace row {ref_index} column {k} ({name}): device {row[k]!r}, reference {ref_row[k]!r}")


def root_sum(r: float) -> float:
    """a double s with sqrt(s) == r exactly (nextafter of r * r is not enough: its root still rounds to the old value)"""
    r = float(r)
    s = r * r
    while math.sqrt(s) > r:
        s = math.nextafter(s, 0.0)
    while math.sqrt(s) < r:
        s = math.nextafter(s, math.inf)
    assert math.sqrt(s) == r
    return s


def _control_table():
    """Crafted sums for the control step: (name, params, [sums of each step in turn]).  rho = 1, nu = 10: s0 = 400, s1 = 2 gives
    pri = 20 = nu dual exactly; mirrored (s0 = 4, s1 = 200) for the decrease.  'below': the nearest sums whose square ROOT is one ulp
    lower.  Every step of a sequence is checked, the last is the one the name speaks of.  tau_incr = 3, tau_decr = 2 throughout, so
    that the decrease branch's mu rescale by tau_incr is pinned."""
    P = lambda **kw: control_params(tau_incr=3.0, tau_decr=2.0, **kw)
    lo = math.nextafter(20.0, 0.0)
    rest = [1.0, 1.0, 1.0]
    neutral = [4.0, 2.0] + rest                       # pri = dual = 2: no branch, no stop
    incr, decr = [400.0, 2.0] + rest, [4.0, 200.0] + rest
    t = [
        ("increase_at_boundary", P(), [incr]),
        ("increase_one_ulp_below", P(), [[root_sum(lo), 2.0] + rest]),
        ("decrease_at_boundary", P(), [decr]),
        ("decrease_one_ulp_below", P(), [[4.0, root_sum(lo) / 2.0] + rest]),
        ("increase_then_decrease", P(), [incr, decr, neutral]),
        ("both_zero_increase_wins_and_converges", P(), [[0.0, 0.0] + rest]),
        ("rho_limit_minus_one_adapts", P(it_rho_limit=3), [neutral, incr]),
        ("rho_limit_reached_no_increase", P(it_rho_limit=3), [neutral, neutral, incr]),
        ("rho_limit_reached_no_decrease", P(it_rho_limit=3), [neutral, neutral, decr]),
        ("max_it_then_gated", P(max_it=2), [neutral, neutral, incr]),
        ("max_it_one", P(max_it=1), [decr]),
        ("inf_sum", P(), [neutral, [math.inf, 2.0] + rest, neutral]),
        ("nan_sum", P(), [neutral, [4.0, 2.0, math.nan, 1.0, 1.0], neutral]),
        ("overflowing_total", P(), [[1.5e308, 1.5e308] + rest, neutral]),
        ("largest_finite_total_is_not_diverged", P(), [[1.75e308, 0.0] + rest, [0.0, 8.9e307] + rest]),
        ("converged_without_rho_change", P(), [neutral, [1e-12, 5e-13, 1.0, 1.0, 1.0], incr]),
        ("converged_with_rho_increase", P(), [neutral, [1e-10, 0.0, 1.0, 1.0, 1.0]]),
        ("converged_with_rho_decrease", P(), [neutral, [0.0, 1e-10, 1.0, 1.0, 1.0]]),
        ("start_rho_64_decrease", P(rho=64.0), [[4.0, 200.0 / 4096.0] + rest, [4.0, root_sum(lo) / 2.0 / 1024.0] + rest]),
        ("large_norms_relative_eps", P(), [[9.0, 3.0, 1e4, 2e4, 5e3], [1e4, 3.0, 1e4, 2e4, 5e3]]),
    ]
    return t


CONTROL_TABLE = _control_table()


# -------------------------------------------------------------------------------------------------
# cost
# -------------------------------------------------------------------------------------------------
def cost_reference(zv, zedge, n, eps_edge, edge_counted=None):
    """(cost, sum of the absolute terms): sum_v |z_v[:n] - z_v[n:]| + eps_edge sum_e w_e y_e, y_e = the last word of zedge"""
    zv = np.asarray(zv, dtype=np.float64)
    d = _wide(zv[:, :n]) - _wide(zv[:, n:2 * n])
    length = np.sqrt(np.sum(d * d, axis=1))
    we = 1.0 if edge_counted is None else _wide(np.asarray(edge_counted).astype(np.float64))
    pen = _wide(float(eps_edge)) * we * _wide(np.asarray(zedge)[2 * n].astype(np.float64))
    terms = np.concatenate([np.asarray(length).ravel(), np.asarray(pen).ravel()])
    return _total(terms), _total(np.abs(terms))


def cost_bound(V, E, n, abs_terms) -> float:
    return (V * (n + 2) + E + 8) * EPS53 * abs_terms


def check_cost(case, ref, abs_terms, dev, V, E, n):
    bound = cost_bound(V, E, n, abs_terms)
    if not abs(float(dev) - ref) <= bound:
        raise AssertionError(f"{case}: cost: device {float(dev)!r}, reference {ref!r}, difference {abs(float(dev) - ref):.3e}, bound {bound:.3e}")
    return abs(float(dev) - ref) / bound if bound else 0.0


def random_edge_state(seed, c, NI, E, dtype):
    """(copy [c, NI], zedge [c, E], mu [c, NI]) standard normal in the state type, with a few columns scaled by 1e+6 and 1e-6 so
    that a value read from the wrong column is not hidden among equals"""
    rng = np.random.default_rng(seed)
    copy, zedge, mu = rng.standard_normal((c, NI)), rng.standard_normal((c, E)), rng.standard_normal((c, NI))
    for a, n in ((copy, NI), (mu, NI), (zedge, E)):
        k = max(1, n // 97)
        a[:, rng.choice(n, size=k, replace=False)] *= 1e6
        a[:, rng.choice(n, size=k, replace=False)] *= 1e-6
    dt = np.dtype(dtype)
    return copy.astype(dt), zedge.astype(dt), mu.astype(dt)


# -------------------------------------------------------------------------------------------------
# the cases of the GPU edge-step table (tests/test_gpu_edge_control.py) and the launch each is there for
# (pinned against the host plan by tests/test_loop_reference.py)
# -------------------------------------------------------------------------------------------------
EDGE_BLOCK, EDGE_BLOCKS_MAX = 256, 2048      # csrc/create_plan.h


class EdgeCase:
    """graph: ('chain', k) | ('lattice', nx, ny, n, seed) | ('fixture', name); partition: None or (rank, world);
    expect: (E, edge_unroll, edge_blocks, second pass of the grid-stride loop)"""

    def __init__(self, name, graph, dtype, columns, partition, expect, why, big=False):
        self.name, self.graph, self.dtype, self.columns, self.partition = name, graph, dtype, columns, partition
        self.expect, self.why, self.big = expect, why, big

    @property
    def id(self):
        return f"{self.name}-{self.dtype}-{self.columns}"

    def build(self, cache=None):
        """(GcsGraph to hand to the solver, LocalPartition or None); ``cache``: dict that keeps the full graphs"""
        from gcs_admm_amd.graph import graph_from_sets, lattice_boxes
        key = self.graph
        g = cache.get(key) if cache is not None else None
        if g is None:
            if key[0] == "chain":
                from conftest import interval_chain
                g = graph_from_sets(*interval_chain(key[1]))
            elif key[0] == "fixture":
                from gcs_admm_amd.cases import load_fixture
                g = load_fixture(key[1])[1]
            else:
                g = lattice_boxes(key[1], key[2], n=key[3], seed=key[4])
            if cache is not None:
                cache[key] = g
        if self.partition is None:
            return g, None
        from gcs_admm_amd.partition import build_partition, strip_owner
        rank, world = self.partition
        p = build_partition(g, strip_owner(g, world), rank, world)
        return p.graph, p


def _tiles(E, U):
    return -(-E // (EDGE_BLOCK * U))


def _edge_cases():
    L = lambda nx, ny, n=2, seed=1: ("lattice", nx, ny, n, seed)
    C = EdgeCase
    cases = [
        # all eight C instantiations, both types; E below a wavefront, between one and four, several workgroups
        C("chain_n1", ("chain", 8), "f64", "incidence", None, (18, 1, 1, False), "C = 3, E < 64"),
        C("chain_n1", ("chain", 8), "f32", "incidence", None, (18, 1, 1, False), "C = 3, E < 64"),
        C("lattice_n2_3x3", L(3, 3), "f64", "incidence", None, (24, 1, 1, False), "C = 5, E < 64"),
        C("lattice_n2_3x3", L(3, 3), "f32", "incidence", None, (24, 1, 1, False), "C = 5, E < 64"),
        C("lattice_n3_6x5", L(6, 5, 3), "f64", "incidence", None, (92, 1, 1, False), "C = 7, 64 < E < 256"),
        C("lattice_n3_6x5", L(6, 5, 3), "f32", "incidence", None, (92, 1, 1, False), "C = 7, 64 < E < 256"),
        C("lattice_n4_12x10", L(12, 10, 4), "f64", "incidence", None, (418, 1, 2, False), "C = 9, two workgroups"),
        C("lattice_n4_12x10", L(12, 10, 4), "f32", "incidence", None, (418, 1, 2, False), "C = 9, two workgroups"),
        C("lattice_n5_4x3", L(4, 3, 5), "f64", "incidence", None, (32, 1, 1, False), "C = 11, E < 64"),
        C("lattice_n5_4x3", L(4, 3, 5), "f32", "incidence", None, (32, 1, 1, False), "C = 11, E < 64"),
        C("lattice_n6_7x6", L(7, 6, 6), "f64", "incidence", None, (134, 1, 1, False), "C = 13, 64 < E < 256"),
        C("lattice_n6_7x6", L(7, 6, 6), "f32", "incidence", None, (134, 1, 1, False), "C = 13, 64 < E < 256"),
        C("lattice_n7_19x17", L(19, 17, 7), "f64", "incidence", None, (1188, 1, 5, False), "C = 15, five workgroups"),
        C("lattice_n7_19x17", L(19, 17, 7), "f32", "incidence", None, (1188, 1, 5, False), "C = 15, five workgroups"),
        C("lattice_n8_6x5", L(6, 5, 8), "f64", "incidence", None, (92, 1, 1, False), "C = 17, 64 < E < 256"),
        C("lattice_n8_6x5", L(6, 5, 8), "f32", "incidence", None, (92, 1, 1, False), "C = 17, 64 < E < 256"),
        # fixtures: one workgroup, a nearly empty wavefront
        C("benchmark4", ("fixture", "benchmark4"), "f64", "incidence", None, (94, 1, 1, False), "single workgroup"),
        C("test1", ("fixture", "test1"), "f64", "incidence", None, (4, 1, 1, False), "four edges"),
        # null index arrays
        C("lattice_n2_23x21", L(23, 21), "f64", "edge", None, (1804, 1, 8, False), "edge-major columns, several workgroups"),
        C("lattice_n3_6x5", L(6, 5, 3), "f32", "edge", None, (92, 1, 1, False), "edge-major columns, one workgroup"),
        # ghost columns and ownership masks, both column orders, both ranks' shapes
        C("lattice_n2_14x16_part0of2", L(14, 16, 2, 5), "f64", "incidence", (0, 2), (434, 1, 2, False), "masks, NI > NI_owned"),
        C("lattice_n2_14x16_part1of2", L(14, 16, 2, 5), "f32", "incidence", (1, 2), (434, 1, 2, False), "masks, NI > NI_owned"),
        C("lattice_n2_14x16_part0of2", L(14, 16, 2, 5), "f32", "edge", (0, 2), (434, 1, 2, False), "masks, edge-major"),
        C("lattice_n2_14x16_part1of2", L(14, 16, 2, 5), "f64", "edge", (1, 2), (434, 1, 2, False), "masks, edge-major"),
        # unrolled tiles and their clamped tail
        C("lattice_100k", L(316, 317, 2, 0), "f64", "incidence", None, (398796, 2, 779, False), "U = 2", big=True),
        C("lattice_100k", L(316, 317, 2, 0), "f32", "incidence", None, (398796, 4, 390, False), "U = 4", big=True),
        # the second pass of the grid-stride loop (more tiles than the 2048 workgroups)
        C("lattice_520", L(520, 520, 2, 0), "f64", "incidence", None, (1078486, 2, 2048, True), "U = 2 and second pass", big=True),
        C("lattice_730", L(730, 730, 2, 0), "f32", "incidence", None, (2127226, 4, 2048, True), "U = 4 and second pass", big=True),
        C("lattice_370_n4", L(370, 370, 4, 0), "f64", "incidence", None, (545386, 1, 2048, True), "U = 1 and second pass", big=True),
        C("lattice_370_n4", L(370, 370, 4, 0), "f32", "incidence", None, (545386, 2, 1066, False), "C > 7: U = 2", big=True),
    ]
    return cases


EDGE_CASES = _edge_cases()
