"""tests/loop_reference.py on the CPU: the numpy restatement of the edge step, the loop control and the cost against the C oracle
(this checks the oracle as much as the reference), the checkers against seeded faults, and the launch every case of the GPU
table (tests/test_gpu_edge_control.py) is there for against the host plan.

Seeded faults.  For each one the test states -- and asserts -- what the criteria the suite had before would have said of the same
outputs: ``old_sums`` = the five sums within rtol 1e-9 of a recomputation (the lattice property tests), ``old_trace`` = pri and dual
within 2e-4 + 1e-3 |ref| of the reference (every whole-run comparison; the only check the fused launches had).  The contract of
loop_reference.py rejects all of them."""
import math

import numpy as np
import pytest

import loop_reference as lr
from conftest import interval_chain  # noqa: F401  (EdgeCase.build imports it the same way)
from gcs_admm_amd import IPM_TOL
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import lattice_boxes
from gcs_admm_amd.partition import build_partition, strip_owner

FORCED = (0.5, 2.0, 1.0 / 3.0, 3.0)
TAU_INCR, TAU_DECR = 3.0, 2.0


def test_extended_precision_is_available():
    """the reference sums want a 64-bit mantissa (x86 long double); without one they fall back to math.fsum, which is exact"""
    assert lr.LONGDOUBLE_OK or math.fsum([1.0, 1e-30, -1.0]) == 1e-30
    assert lr.root_sum(math.nextafter(20.0, 0.0)) < math.nextafter(400.0, 0.0)       # why nextafter(400, 0) is not enough
    assert math.sqrt(math.nextafter(400.0, 0.0)) == 20.0


# -------------------------------------------------------------------------------------------------
# the reference against the oracle, along the oracle's own loop
# -------------------------------------------------------------------------------------------------
def _oracles(oracle_lib, name):
    """[(oracle, inc_counted, edge_counted)], the halo exchange between them, nx, nmu"""
    if name == "two_partitions":
        g = lattice_boxes(12, 16, seed=5)
        owner = strip_owner(g, 2)
        parts = [build_partition(g, owner, r, 2) for r in range(2)]
        os_ = [oracle_lib.Oracle(p.graph, ipm_tol=IPM_TOL, num_incidences=p.num_incidences, inc_counted=p.inc_counted,
                                 edge_counted=p.edge_counted, nx_global=p.nx_global, nmu_global=p.nmu_global) for p in parts]

        def exchange():
            for r in range(2):
                o = 1 - r
                os_[r].copy[:, parts[r].recv_idx[o]] = os_[o].copy[:, parts[o].send_idx[r]]
        assert any(p.num_incidences > int(p.graph.inc_ptr[-1]) for p in parts)
        return [(o, p.inc_counted, p.edge_counted) for o, p in zip(os_, parts)], exchange, float(g.nx), float(g.nmu)
    g = {"lattice_60": lambda: lattice_boxes(60, 60, seed=0), "lattice_n3": lambda: lattice_boxes(9, 8, n=3, seed=2)}.get(
        name, lambda: load_fixture(name)[1])()
    return [(oracle_lib.Oracle(g, ipm_tol=IPM_TOL), None, None)], (lambda: None), float(g.nx), float(g.nmu)


@pytest.mark.parametrize("name,rho", [("benchmark1", 1.0), ("benchmark1", 64.0), ("benchmark4", 1.0), ("benchmark4", 1.0 / 64.0),
                                      ("lattice_60", 1.0), ("lattice_n3", 1.0), ("two_partitions", 1.0)])
def test_reference_against_oracle_along_a_run(oracle_lib, name, rho):
    """20 iterations of the oracle's loop with tau_incr = 3, tau_decr = 2: every edge step -- with the loop's own mu_scale and,
    from the same state, with mu_scale forced to 1/2, 2, 1/3, 3 -- and every control step against the reference.  The oracle is
    built without fma contraction, so zedge, mu, the control state and the trace row are bitwise; the sums meet their bound."""
    oracles, exchange, nx, nmu = _oracles(oracle_lib, name)
    ap = oracle_lib._Admm(rho, TAU_INCR, TAU_DECR, 10.0, 100, 1e-4, 1e-3, 1000)
    params = lr.control_params(TAU_INCR, TAU_DECR, 10.0, 100, 1000, 1e-4, 1e-3, rho)
    state = np.array([rho, 1.0, 1.0, -1.0])
    cb = lr.control_block(rho=rho)
    scales, worst = set(), 0.0
    for it in range(20):
        fails = sum(o.vertex_step(rho=state[0], mu_scale=state[1]) for o, _, _ in oracles)
        exchange()
        total = np.zeros(5)
        for k, (o, ic, ec) in enumerate(oracles):
            z0, mu0 = o.zedge.copy(), o.mu.copy()
            tail, head = o.g.edge_inc_tail, o.g.edge_inc_head
            for ms in FORCED + (float(state[1]),):          # the loop's own last: its result stays
                o.zedge[...] = z0; o.mu[...] = mu0
                s = o.edge_step(ms)
                ref = lr.edge_reference(tail, head, o.copy, z0, mu0, ms, ic, ec)
                st = lr.check_edge_step(f"{name} rho {rho} it {it} part {k} mu_scale {ms!r}", ref, o.zedge, o.mu, s)
                assert st["mu_bitwise"], (name, it, ms)
                worst = max(worst, st["worst_sum"])
            total += s
        scales.add(float(state[1]))
        row = np.full(6, -7.0)
        oracles[0][0].control(ap, total, state, float(fails), row)
        ref_cb, ref_row, _ = lr.control_reference(cb, total, params, nx, nmu, fails)
        dev = lr.control_block(state[0], state[1], int(state[2]), int(state[3]), fails, total, row[1], row[2], row[3], row[4])
        lr.check_control(f"{name} rho {rho} it {it}", ref_cb, ref_row, 0, dev, np.full((1, 6), -7.0), row[None, :])
        assert np.array_equal(row, ref_row)                  # no contraction on either side: bit for bit
        cb = ref_cb
        assert cb["status"] == lr.RUNNING and cb["it"] == it + 2
    print(f"{name} rho {rho}: worst sum error {worst:.3f} of its bound, mu_scale seen {sorted(scales)}")
    assert worst <= 1.0
    if rho == 64.0:
        assert TAU_INCR in scales             # a decrease rescales mu by tau_incr
    if rho == 1.0 / 64.0:
        assert 1.0 / TAU_INCR in scales


# -------------------------------------------------------------------------------------------------
# the control table against oracle_control
# -------------------------------------------------------------------------------------------------
EXPECTED_END = {      # what each sequence is there to reach: (rho, mu_scale, it, status) after its last step
    "increase_at_boundary": (3.0, 1.0 / 3.0, 2, lr.RUNNING),
    "increase_one_ulp_below": (1.0, 1.0, 2, lr.RUNNING),
    "decrease_at_boundary": (0.5, 3.0, 2, lr.RUNNING),
    "decrease_one_ulp_below": (1.0, 1.0, 2, lr.RUNNING),
    "increase_then_decrease": (1.5, 1.0, 4, lr.RUNNING),
    "both_zero_increase_wins_and_converges": (3.0, 1.0 / 3.0, 1, lr.CONVERGED),
    "rho_limit_minus_one_adapts": (3.0, 1.0 / 3.0, 3, lr.RUNNING),
    "rho_limit_reached_no_increase": (1.0, 1.0, 4, lr.RUNNING),
    "rho_limit_reached_no_decrease": (1.0, 1.0, 4, lr.RUNNING),
    "max_it_then_gated": (1.0, 1.0, 3, lr.MAX_IT),
    "max_it_one": (0.5, 3.0, 2, lr.MAX_IT),
    "inf_sum": (1.0, 1.0, 2, lr.DIVERGED),
    "nan_sum": (1.0, 1.0, 2, lr.DIVERGED),
    "overflowing_total": (1.0, 1.0, 1, lr.DIVERGED),
    "largest_finite_total_is_not_diverged": (1.5, 3.0, 3, lr.RUNNING),      # (2 s1 = 1.78e308 is still finite: dual = 3 sqrt(2 s1))
    "converged_without_rho_change": (1.0, 1.0, 2, lr.CONVERGED),
    "converged_with_rho_increase": (3.0, 1.0 / 3.0, 2, lr.CONVERGED),
    "converged_with_rho_decrease": (0.5, 3.0, 2, lr.CONVERGED),
    "start_rho_64_decrease": (32.0, 1.0, 3, lr.RUNNING),
    "large_norms_relative_eps": (3.0, 1.0 / 3.0, 3, lr.RUNNING),
}


def test_control_table_is_complete():
    assert [t[0] for t in lr.CONTROL_TABLE] == list(EXPECTED_END)


@pytest.mark.parametrize("entry", lr.CONTROL_TABLE, ids=[t[0] for t in lr.CONTROL_TABLE])
def test_control_reference_against_oracle_control(oracle_lib, entry):
    name, p, steps = entry
    g = load_fixture("benchmark4")[1]
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL)
    ap = oracle_lib._Admm(p["rho"], p["tau_incr"], p["tau_decr"], p["nu"], p["it_rho_limit"], p["eps_abs"], p["eps_rel"], p["max_it"])
    state = np.array([p["rho"], 1.0, 1.0, -1.0])
    cb = lr.control_block(rho=p["rho"])
    for k, sums in enumerate(steps):
        fails = k + 3
        row = np.full(6, -7.0)
        o.control(ap, np.array(sums), state, float(fails), row)
        ref_cb, ref_row, _ = lr.control_reference(cb, sums, p, float(g.nx), float(g.nmu), fails)
        what = f"{name} step {k}"
        assert (state[0], state[1], int(state[2]), int(state[3])) == (ref_cb["rho"], ref_cb["mu_scale"], ref_cb["it"], ref_cb["status"]), what
        if ref_row is None:
            assert np.all(row == -7.0), what
        else:
            assert np.array_equal(row, ref_row), what
        cb = ref_cb
    assert (cb["rho"], cb["mu_scale"], cb["it"], cb["status"]) == EXPECTED_END[name]


# -------------------------------------------------------------------------------------------------
# seeded faults
# -------------------------------------------------------------------------------------------------
def _model_edge_step(tail, head, copy, z_old, mu_old, mu_scale, ic, ec, fault=None, nblocks=2048):
    """a device as the kernel is written -- double arithmetic, per-workgroup partials, a final reduction -- with one seeded fault"""
    c, E = z_old.shape
    cu, cw = copy[:, tail], copy[:, head]
    zn = 0.5 * (cu + cw)
    if fault == "stale_zedge":
        zn[:, E // 3] = z_old[:, E // 3]
    ru, rw = cu - zn, cw - zn
    ms = 1.0 if fault == "mu_without_scale" else mu_scale
    mu = mu_old.copy()
    mu[:, tail] = ms * mu_old[:, tail] + ru
    mu[:, head] = ms * mu_old[:, head] + rw
    if fault == "columns_swapped":
        e = (2 * E) // 3
        mu[:, tail[e]] = ms * mu_old[:, head[e]] + rw[:, e]
        mu[:, head[e]] = ms * mu_old[:, tail[e]] + ru[:, e]
    masks = fault != "masks_ignored"
    wt = ic[tail].astype(float) if ic is not None and masks else np.ones(E)
    wh = ic[head].astype(float) if ic is not None and masks else np.ones(E)
    we = ec.astype(float) if ec is not None and masks else np.ones(E)
    mu_u, mu_w = mu[:, tail], mu[:, head]
    dz = zn - (zn if fault == "sum1_against_new" else z_old)
    per_edge = np.stack([(wt * ru * ru + wh * rw * rw).sum(0), (we * dz * dz).sum(0), (wt * cu * cu + wh * cw * cw).sum(0),
                         (we * zn * zn).sum(0), (wt * mu_u * mu_u + wh * mu_w * mu_w).sum(0)])
    if fault == "last_37_edges":
        per_edge = per_edge[:, :E - 37]
    partials = np.stack([b.sum(1) for b in np.array_split(per_edge, nblocks, axis=1)])
    sums = partials.sum(0)
    if fault == "partial_twice":
        sums = sums + partials[nblocks // 2]
    return zn, mu, sums


def _old_criteria(ref_sums, dev_sums, rho=1.0):
    old_sums = bool(np.allclose(dev_sums, ref_sums, rtol=1e-9, atol=0.0))
    res = lambda s: np.array([math.sqrt(s[0]), rho * math.sqrt(2.0 * s[1])])
    a, b = res(dev_sums), res(ref_sums)
    return old_sums, bool(np.all(np.abs(a - b) <= 2e-4 + 1e-3 * np.abs(b)))


@pytest.fixture(scope="module")
def fault_bench():
    """a realistic state: the two-million-word edge step of a 210 x 210 lattice, 12 oracle-free iterations in (random state of the
    size of a converging run's: copies O(100), duals O(1)), and one partition of it for the masks"""
    g = lattice_boxes(210, 210, seed=4)
    E, c, NI = g.num_edges, g.c, 2 * g.num_edges
    rng = np.random.default_rng(11)
    base = rng.uniform(0.0, 200.0, size=(c, E))
    copy = np.empty((c, NI)); copy[:, g.edge_inc_tail] = base + 0.01 * rng.standard_normal((c, E)); copy[:, g.edge_inc_head] = base + 0.01 * rng.standard_normal((c, E))
    z_old = base + 0.01 * rng.standard_normal((c, E))
    mu_old = rng.standard_normal((c, NI))
    p = build_partition(g, strip_owner(g, 2), 0, 2)
    return g, copy, z_old, mu_old, p


EDGE_FAULTS = [      # fault, old_sums passes, old_trace passes
    ("stale_zedge", False, True),
    ("mu_without_scale", False, True),          # (sum 4 moves; pri and dual do not see mu at all)
    ("columns_swapped", True, True),             # (the sums are symmetric in the two columns: only mu shows it)
    ("last_37_edges", False, True),
    ("partial_twice", False, True),
    ("sum1_against_new", False, False),         # dual = 0: the one fault of this list a whole-run trace shows
]


def test_checker_accepts_the_clean_model(fault_bench):
    g, copy, z_old, mu_old, p = fault_bench
    tail, head = g.edge_inc_tail, g.edge_inc_head
    for ms in (1.0, 1.0 / 3.0):
        ref = lr.edge_reference(tail, head, copy, z_old, mu_old, ms)
        z, mu, sums = _model_edge_step(tail, head, copy, z_old, mu_old, ms, None, None)
        st = lr.check_edge_step(f"clean mu_scale {ms!r}", ref, z, mu, sums)
        assert st["mu_bitwise"] and st["worst_sum"] <= 1.0
        assert _old_criteria(ref["sums"], sums) == (True, True)


@pytest.mark.parametrize("fault,old_sums,old_trace", EDGE_FAULTS, ids=[f[0] for f in EDGE_FAULTS])
def test_checker_rejects_edge_faults(fault_bench, fault, old_sums, old_trace):
    g, copy, z_old, mu_old, p = fault_bench
    tail, head = g.edge_inc_tail, g.edge_inc_head
    ms = 1.0 / 3.0
    ref = lr.edge_reference(tail, head, copy, z_old, mu_old, ms)
    z, mu, sums = _model_edge_step(tail, head, copy, z_old, mu_old, ms, None, None, fault)
    got = _old_criteria(ref["sums"], sums)
    print(fault, "old criteria (sums rtol 1e-9, trace 2e-4 + 1e-3):", got, "relative sum differences", np.abs(sums - ref["sums"]) / ref["sums"])
    assert got == (old_sums, old_trace)
    with pytest.raises(AssertionError, match="device"):
        lr.check_edge_step(fault, ref, z, mu, sums)


def test_checker_rejects_a_fault_in_zedge_or_mu_with_correct_sums(fault_bench):
    """what only the state comparison sees: the sums handed over are the reference's own, the old criteria have nothing to object to"""
    g, copy, z_old, mu_old, p = fault_bench
    tail, head = g.edge_inc_tail, g.edge_inc_head
    ms = 3.0
    ref = lr.edge_reference(tail, head, copy, z_old, mu_old, ms)
    for fault, needle in (("stale_zedge", "zedge word"), ("mu_without_scale", "mu word"), ("columns_swapped", "mu word")):
        z, mu, _ = _model_edge_step(tail, head, copy, z_old, mu_old, ms, None, None, fault)
        assert _old_criteria(ref["sums"], ref["sums"]) == (True, True)
        with pytest.raises(AssertionError, match=needle):
            lr.check_edge_step(fault, ref, z, mu, ref["sums"])


def test_what_the_mu_bound_says_of_a_contracted_dual_update(fault_bench):
    """mu_scale = 1/3 with mu_scale * mu + r formed as ONE fma (modelled in extended precision).  Such a device differs from the
    reference in a few percent of the words (3 % on this state), never by more than the product's rounding error plus one ulp of mu_new -- and the per-word bound
    2^-53 (|mu_scale mu| + |mu_new|) has room for all of them but the few (a share of about 4e-4 here) whose exact value lies within
    the product's rounding error of a rounding midpoint of mu_new: there the two roundings land on neighbouring doubles, one ulp
    = up to 2^-52 |mu_new| apart, which the bound only covers when |mu_scale mu| is at least |mu_new|.  The checker holds the bound as
    stated, so it asks for a dual update whose product is rounded on its own whenever mu_scale is not a power of two; two ulp are
    outside on any reading.  (On the MI355X the contracted form, which the compiler chooses if left alone, put 4-5 % of the f64 words
    of a standard-normal state outside the bound, and left 2e-17 in an f32 word whose two terms cancel exactly; edge_kernel therefore
    forms the product with contraction off, csrc/edge_step.h scaled_plus.)"""
    if not lr.LONGDOUBLE_OK:
        pytest.skip("models the fma in extended precision")
    g, copy, z_old, mu_old, p = fault_bench
    tail, head = g.edge_inc_tail, g.edge_inc_head
    ms = 1.0 / 3.0
    z, mu, sums = _model_edge_step(tail, head, copy, z_old, mu_old, ms, None, None)
    ref = lr.edge_reference(tail, head, copy, z_old, mu_old, ms)
    L = np.longdouble
    for cols in (tail, head):
        mu[:, cols] = (L(ms) * mu_old[:, cols].astype(L) + (copy[:, cols] - z).astype(L)).astype(np.float64)
    differ = mu != ref["mu"]
    assert 0.005 < differ.mean() < 0.6
    # the product's rounding error and one ulp of the result: what two correct roundings can be apart
    assert np.all(np.abs(mu - ref["mu"]) <= lr.EPS53 * np.abs(ms * mu_old) + np.spacing(np.maximum(np.abs(mu), np.abs(ref["mu"]))))
    outside = np.abs(mu - ref["mu"]) > lr.EPS53 * (np.abs(ms * mu_old) + np.abs(ref["mu"]))
    print(f"contracted dual update: {differ.mean():.3f} of the words differ, {outside.mean():.2e} outside the bound")
    assert 0 < outside.mean() < 2e-3
    with pytest.raises(AssertionError, match="mu word"):
        lr.check_edge_step("contracted", ref, z, mu, sums)
    mu = ref["mu"].copy()
    w, k = 3, int(tail[5])
    mu[w, k] = np.nextafter(ref["mu"][w, k], np.inf)       # one ulp, where the bound has room for it
    if lr.EPS53 * (abs(ms * mu_old[w, k]) + abs(ref["mu"][w, k])) >= np.spacing(abs(ref["mu"][w, k])):
        assert not lr.check_edge_step("one ulp inside", ref, z, mu, sums)["mu_bitwise"]
    mu[w, k] = np.nextafter(np.nextafter(ref["mu"][w, k], np.inf), np.inf)
    with pytest.raises(AssertionError, match="mu word 3"):
        lr.check_edge_step("two ulp", ref, z, mu, sums)


def test_checker_rejects_ignored_masks(fault_bench):
    g, copy, z_old, mu_old, p = fault_bench
    lg = p.graph
    tail, head, NI, E = lg.edge_inc_tail, lg.edge_inc_head, p.num_incidences, lg.num_edges
    cp, zo, mo = lr.random_edge_state(3, lg.c, NI, E, np.float64)
    ref = lr.edge_reference(tail, head, cp, zo, mo, 2.0, p.inc_counted, p.edge_counted)
    z, mu, sums = _model_edge_step(tail, head, cp, zo, mo, 2.0, p.inc_counted, p.edge_counted, None, nblocks=64)
    lr.check_edge_step("clean partition", ref, z, mu, sums)
    z, mu, sums = _model_edge_step(tail, head, cp, zo, mo, 2.0, p.inc_counted, p.edge_counted, "masks_ignored", nblocks=64)
    old = _old_criteria(ref["sums"], sums)
    print("masks_ignored: old criteria", old, np.abs(sums - ref["sums"]) / ref["sums"])
    assert old[0] is False       # (a partition's sums were only ever compared as a total at rtol 1e-3: test_partitioned_handles_match_single)
    with pytest.raises(AssertionError, match="sum 0"):
        lr.check_edge_step("masks_ignored", ref, z, mu, sums)
    # cost without the edge_counted weight
    zv = np.random.default_rng(5).standard_normal((lg.num_vertices, 2 * lg.n))
    zo[2 * lg.n] = np.abs(zo[2 * lg.n]) % 1.0
    ref_cost, abs_terms = lr.cost_reference(zv, zo, lg.n, 1e-4, p.edge_counted)
    good = float(np.sqrt(((zv[:, :lg.n] - zv[:, lg.n:]) ** 2).sum(1)).sum() + 1e-4 * (p.edge_counted * zo[2 * lg.n]).sum())
    lr.check_cost("clean cost", ref_cost, abs_terms, good, lg.num_vertices, E, lg.n)
    faulty = float(np.sqrt(((zv[:, :lg.n] - zv[:, lg.n:]) ** 2).sum(1)).sum() + 1e-4 * zo[2 * lg.n].sum())
    assert abs(faulty - ref_cost) <= 2e-4 * abs(ref_cost)          # the old criterion (2e-4 relative) passes it
    with pytest.raises(AssertionError, match="cost"):
        lr.check_cost("cost without edge_counted", ref_cost, abs_terms, faulty, lg.num_vertices, E, lg.n)


def _model_control(cb, sums, p, nx, nmu, fails, trace, fault=None):
    """control_body as it is written, with one seeded fault; writes ``trace`` in place, returns the new block"""
    out = dict(cb); out["sums"] = np.array(sums, dtype=float); out["inner_failures"] = fails
    if cb["status"] != lr.RUNNING:
        return dict(cb)
    s = out["sums"]
    with np.errstate(over="ignore"):
        total = s.sum()
    if not np.isfinite(total):
        out["status"] = lr.DIVERGED
        return out
    it, rho = cb["it"], cb["rho"]
    limit = p["it_rho_limit"] + (1 if fault == "rho_limit_off_by_one" else 0)
    pri, dual = math.sqrt(s[0]), rho * math.sqrt(2.0 * s[1])
    ge = (lambda a, b: a > b) if fault == "gt_for_ge" else (lambda a, b: a >= b)
    mu_scale = 1.0
    if ge(pri, p["nu"] * dual) and it < limit:
        rho *= p["tau_incr"]; mu_scale = 1.0 / p["tau_incr"]
    elif ge(dual, p["nu"] * pri) and it < limit:
        rho *= 1.0 / p["tau_decr"]; mu_scale = p["tau_decr"] if fault == "decrease_scales_by_tau_decr" else p["tau_incr"]
    eps_pri = math.sqrt(nx) * p["eps_abs"] + p["eps_rel"] * max(math.sqrt(s[2]), math.sqrt(2.0 * s[3]))
    eps_dual = math.sqrt(nmu) * p["eps_abs"] + p["eps_rel"] * (1.0 if fault == "eps_dual_without_scale" else mu_scale) * math.sqrt(s[4])
    out.update(rho=rho, mu_scale=mu_scale, pri=pri, dual=dual, eps_pri=eps_pri, eps_dual=eps_dual)
    trace[it if fault == "trace_row_at_it" else it - 1] = [rho, pri, dual, eps_pri, eps_dual, fails]
    if pri < eps_pri and dual < eps_dual:
        out["status"] = lr.CONVERGED
        return out
    out["it"] = it + 1
    if it + 1 > p["max_it"]:
        out["status"] = lr.MAX_IT
    return out


def _run_model(entry, fault, nx=1e4, nmu=5e3):
    """the table entry through the model and the checker; returns whether the old whole-run criteria (rho, stop iteration and status
    equal; pri, dual of the rows the solver reads within 2e-4 + 1e-3 |ref|) would have accepted the model's outputs"""
    name, p, steps = entry
    cb_ref = lr.control_block(rho=p["rho"]); cb_dev = lr.control_block(rho=p["rho"])
    trace, trace_ref = np.zeros((8, 6)), np.zeros((8, 6))
    rejected = None
    for k, sums in enumerate(steps):
        before = trace.copy()
        new_dev = _model_control(cb_dev, sums, p, nx, nmu, k, trace, fault)
        decide = {f: new_dev[f] for f in lr.CB_ULP}
        ref, row, idx = lr.control_reference(cb_dev, sums, p, nx, nmu, k, decide_on=decide if cb_dev["status"] == lr.RUNNING and np.isfinite(sum(sums)) else None)
        ref_own, row_own, idx_own = lr.control_reference(cb_ref, sums, p, nx, nmu, k)
        if row_own is not None:
            trace_ref[idx_own] = row_own
        cb_ref = ref_own
        if rejected is None:
            try:
                lr.check_control(f"{name} step {k} {fault}", ref, row, idx, new_dev, before, trace)
            except AssertionError as e:
                rejected = str(e)
        cb_dev = new_dev
    rows = min(cb_ref["it"], 8)
    old = (cb_dev["rho"], cb_dev["it"], cb_dev["status"]) == (cb_ref["rho"], cb_ref["it"], cb_ref["status"]) and \
        bool(np.all(np.abs(trace[:rows, 1:3] - trace_ref[:rows, 1:3]) <= 2e-4 + 1e-3 * np.abs(trace_ref[:rows, 1:3])))
    return rejected, old


_ENTRY = {t[0]: t for t in lr.CONTROL_TABLE}
CONTROL_FAULTS = [      # fault, the table entry that shows it, whether the old whole-run criteria accept the faulty outputs ON THAT INPUT
    ("decrease_scales_by_tau_decr", "decrease_at_boundary", True),        # mu_scale was never compared; every old test has tau_incr = tau_decr
    ("gt_for_ge", "increase_at_boundary", False),                         # rho differs -- on an input no old test contains
    ("gt_for_ge", "decrease_at_boundary", False),
    ("rho_limit_off_by_one", "rho_limit_reached_no_increase", False),     # rho differs at it = it_rho_limit, which no old test reaches adapting
    ("rho_limit_off_by_one", "rho_limit_reached_no_decrease", False),
    ("eps_dual_without_scale", "large_norms_relative_eps", True),         # eps_dual was never compared
    ("trace_row_at_it", "increase_then_decrease", False),                 # a shifted trace: the old comparisons see it
]


def test_checker_accepts_the_clean_control_model():
    for entry in lr.CONTROL_TABLE:
        rejected, old = _run_model(entry, None)
        assert rejected is None and old, (entry[0], rejected)


@pytest.mark.parametrize("fault,entry,old_accepts", CONTROL_FAULTS, ids=[f"{f[0]}-{f[1]}" for f in CONTROL_FAULTS])
def test_checker_rejects_control_faults(fault, entry, old_accepts):
    rejected, old = _run_model(_ENTRY[entry], fault)
    print(fault, entry, "->", rejected, "| old criteria accept:", old)
    assert rejected is not None, "the contract let a seeded fault through"
    assert old == old_accepts
    if fault in ("decrease_scales_by_tau_decr", "gt_for_ge", "rho_limit_off_by_one"):
        # away from the boundaries and with tau_incr = tau_decr (all the suite ran before) the faulty model IS the reference
        for name in ("increase_then_decrease", "converged_without_rho_change", "max_it_then_gated"):
            n_, p, steps = _ENTRY[name]
            p = dict(p, tau_incr=2.0, tau_decr=2.0)
            far = [[s[0] * (1.5 if s[0] > s[1] else 1.0), s[1] * (1.5 if s[1] > s[0] else 1.0)] + list(s[2:]) for s in steps]
            assert _run_model((n_, p, far), fault) == (None, True)


# -------------------------------------------------------------------------------------------------
# the launch each case of the GPU table is there for
# -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_lib():
    import test_create_plan as tcp
    return tcp, tcp.load(tcp.build_lib())


@pytest.fixture(scope="module")
def graphs():
    return {}


@pytest.mark.parametrize("case", lr.EDGE_CASES, ids=[c.id for c in lr.EDGE_CASES])
def test_plan_pins_of_the_gpu_cases(plan_lib, graphs, case):
    tcp, lib = plan_lib
    g, p = case.build(graphs)
    kw = dict(columns=case.columns, dtype=0 if case.dtype == "f64" else 1)
    if p is not None:
        kw.update(num_incidences=p.num_incidences, nx_global=p.nx_global, nmu_global=p.nmu_global)
        assert p.num_incidences > int(g.inc_ptr[-1]) and p.inc_counted.min() == 0 and p.edge_counted.min() == 0      # ghosts and masks
    pl = tcp.plan(lib, g, **kw)
    second_pass = lr._tiles(g.num_edges, pl.edge_unroll) > pl.edge_blocks
    assert (g.num_edges, pl.edge_unroll, pl.edge_blocks, second_pass) == case.expect, case.why
    assert pl.edge_blocks <= lr.EDGE_BLOCKS_MAX
    if case.big:
        assert g.num_edges % (lr.EDGE_BLOCK * pl.edge_unroll) != 0          # the last tile is partial: the clamped tail runs


def test_gpu_cases_cover_every_instantiation():
    """2 types x 8 word counts at U = 1; the unrolled kernels U = 2 (f64 C <= 7, f32 C > 7) and U = 4 (f32 C <= 7); a second pass of
    the grid-stride loop at U = 1, 2 and 4"""
    seen = {(c.dtype, 2 * (1 if c.graph[0] == "chain" else 2 if c.graph[0] == "fixture" else c.graph[3]) + 1, c.expect[1]) for c in lr.EDGE_CASES}
    for dt in ("f64", "f32"):
        for C in (3, 5, 7, 9, 11, 13, 15, 17):
            assert (dt, C, 1) in seen, (dt, C)
    assert {("f64", 5, 2), ("f32", 5, 4), ("f32", 9, 2), ("f64", 9, 1), ("f32", 9, 1)} <= seen
    assert {c.expect[1] for c in lr.EDGE_CASES if c.expect[3]} == {1, 2, 4}
