"""The non-vertex half of the ADMM iteration on the device -- edge_kernel in every launch mode, finalize_kernel, control_body,
cost_kernel (csrc/loop_kernels.h, launched by csrc/gcsadmm.hip) -- against the plain numpy restatement of tests/loop_reference.py, to the bounds derived there:
zedge bitwise, mu bitwise (a stated per-word bound when mu_scale is not a power of two), the five sums within (N + 8) 2^-53
relative, the control block's decisions exact and its residuals within 4 ulp, the cost within its rounding bound.

  (a) the edge step alone (MODE 0 + finalize_kernel) from a seeded random state at mu_scale 1, 1/2, 2, 1/3, 3 over the case table of
      loop_reference.EDGE_CASES: all eight word counts, both state types, edge-major columns, ghost columns with ownership masks,
      the unrolled tiles with their clamped tail, and the second pass of the grid-stride loop (more than 2048 tiles), which no
      other test and no benchmark workload runs.  tests/test_loop_reference.py pins the launch of every case against the host plan.
  (b) the fused launches: MODE 1 (one workgroup, control fused), MODE 2 (last-workgroup ticket reduction + control) and MODE 3 +
      control_kernel (the partitioned loop, serial and overlapped), per iteration from a snapshot; and the same edge step replayed in
      MODE 0 on a second handle: the sums of the fused launches equal MODE 0's bit for bit (the fixed reduction order), zedge and
      mu with them.  The ticket is left usable: two launches of one iteration equal one launch of two.
  (c) the control step alone over the crafted table (both >= boundaries and the sums one ulp of the ROOT below them, tau_incr !=
      tau_decr, it_rho_limit, max_it, non-finite sums -> DIVERGED), and the inner-failure count on both loops.
  (d) the status gate: once the status has left RUNNING no entry point changes the state, the control block or the trace.
  (e) the cost of the device's own last iterate.

Every figure a report wants is printed (run with -s): LOOPREF lines.  Measured on the MI355X: mu bitwise in every case and at every
scale, f64 and f32; the worst sum at 0.042 of its bound (test1, four edges), below 1e-3 of it from 400 edges up and below 1e-6 of it
on the four large lattices (the bound is the worst case of N roundings, the kernel's tree sums do far better); MODE 1 / 2 / 3 sums,
zedge and mu equal MODE 0's bits in every checked iteration; the cost within 0.003 of its bound.  With the dual update left to the
compiler's fma contraction (the kernel before this module existed) 4-5 % of the f64 mu words were outside their bound at mu_scale 1/3
and 3, and an f32 word whose two terms cancel exactly held 2e-17 instead of 0."""
import numpy as np
import pytest

import loop_reference as lr
from gcs_admm_amd.cases import load_fixture
from gcs_admm_amd.graph import lattice_boxes

pytestmark = pytest.mark.gpu

INCR, DECR, NEUTRAL = [400.0, 0.0, 1.0, 1.0, 1.0], [0.0, 200.0, 1.0, 1.0, 1.0], [4.0, 2.0, 1.0, 1.0, 1.0]
# mu_scale -> (tau_incr, crafted sums of the control step that leaves it): dual = 0 / pri = 0 takes the branch at any rho
SCALES = {1.0: (2.0, None), 0.5: (2.0, INCR), 2.0: (2.0, DECR), 1.0 / 3.0: (3.0, INCR), 3.0: (3.0, DECR)}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def graphs():
    """the large graphs are built once"""
    return {}


def _np(t):
    return t.detach().cpu().numpy()


def _handle(g, p, dtype, columns, **kw):
    from gcs_admm_amd.solver import DeviceSolver
    if p is not None:
        kw.update(num_incidences=p.num_incidences, inc_counted=p.inc_counted, edge_counted=p.edge_counted,
                  nx_global=p.nx_global, nmu_global=p.nmu_global)
    return DeviceSolver(g, dtype, device=0, columns=columns, **kw)


def _layout(d, g, p):
    """tail, head, inc_counted, edge_counted in the numbering of the handle's state columns"""
    E = g.num_edges
    if d.edge_major:
        tail, head = np.arange(E), E + np.arange(E)
    else:
        tail, head = g.edge_inc_tail.astype(np.int64), g.edge_inc_head.astype(np.int64)
    ic = ec = None
    if p is not None:
        ic = np.empty(d.NI, dtype=np.uint8); ic[d.col_of] = p.inc_counted
        ec = np.asarray(p.edge_counted, dtype=np.uint8)
    return tail, head, ic, ec


def _set_mu_scale(torch, d, want, **reset_kw):
    """a control block with mu_scale = want: reset, then (unless 1) one control step on crafted sums"""
    tau_incr, sums = SCALES[want]
    d.reset(tau_incr=tau_incr, tau_decr=2.0, zero_state=False, **reset_kw)
    if sums is not None:
        d.control(torch.tensor(sums, dtype=torch.float64, device=d.device))
    cb = d.read_control()
    assert cb.mu_scale == want and cb.status == lr.RUNNING, (want, cb.mu_scale, cb.status)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _first_diff(a, b):
    bad = lr._bits(np.asarray(a)) != lr._bits(np.asarray(b))
    return (lr._first(bad), int(bad.sum())) if bad.any() else None


# -------------------------------------------------------------------------------------------------
# (a) the edge step alone
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lr.EDGE_CASES, ids=[c.id for c in lr.EDGE_CASES])
def test_edge_step_mode0(torch_gpu, graphs, case):
    torch = torch_gpu
    g, p = case.build(graphs)
    assert g.num_edges == case.expect[0]
    d = _handle(g, p, case.dtype, case.columns)
    tail, head, ic, ec = _layout(d, g, p)
    npdt = np.float64 if case.dtype == "f64" else np.float32
    copy, zedge, mu = lr.random_edge_state(1234 + g.num_edges, g.c, d.NI, g.num_edges, npdt)
    worst, off, bitwise = 0.0, 0.0, True
    for ms in SCALES:
        _set_mu_scale(torch, d, ms, eps_abs=0.0, eps_rel=0.0)
        d.copy.copy_(torch.from_numpy(copy)); d.zedge.copy_(torch.from_numpy(zedge)); d.mu.copy_(torch.from_numpy(mu))
        sums = _np(d.edge_step())
        what = f"{case.id} MODE 0 U={case.expect[1]} blocks={case.expect[2]} mu_scale={ms!r}"
        assert _same_bits(_np(d.copy), copy), f"{what}: the edge step wrote copy (first {_first_diff(_np(d.copy), copy)})"
        ref = lr.edge_reference(tail, head, copy, zedge, mu, ms, ic, ec, npdt)
        st = lr.check_edge_step(what, ref, _np(d.zedge), _np(d.mu), sums)
        print(f"LOOPREF edge {what}: worst sum {st['worst_sum']:.2e} of its bound, mu bitwise {st['mu_bitwise']}, "
              f"mu words off {st['mu_off_share']:.3e}")
        worst = max(worst, st["worst_sum"]); off = max(off, st["mu_off_share"]); bitwise = bitwise and st["mu_bitwise"]
    d.close()
    print(f"LOOPREF edge-case {case.id} (E {g.num_edges}, U {case.expect[1]}, blocks {case.expect[2]}, second pass {case.expect[3]}): "
          f"worst sum {worst:.2e} of its bound, mu bitwise at every scale {bitwise}, largest share of mu words off {off:.3e}")


# -------------------------------------------------------------------------------------------------
# (b) the fused launches
# -------------------------------------------------------------------------------------------------
def _fixture_graph(name):
    return load_fixture(name)[1]


FUSED = [
    # id, graph, dtype, columns, mode, reset parameters, warm-up iterations, what precedes each checked iteration
    ("benchmark4-mode1", lambda: _fixture_graph("benchmark4"), "f64", "incidence", 1, dict(), 6, ["plain", "incr", "plain", "decr", "plain"]),
    ("benchmark4-rho1/64-mode1", lambda: _fixture_graph("benchmark4"), "f64", "incidence", 1, dict(rho=1.0 / 64.0), 0, ["plain"] * 5),
    ("benchmark1-rho64-mode1", lambda: _fixture_graph("benchmark1"), "f64", "incidence", 1, dict(rho=64.0), 0, ["plain"] * 8),
    ("lattice10k-f64-mode2", lambda: lattice_boxes(100, 100, seed=0), "f64", "incidence", 2, dict(), 6, ["plain", "incr", "plain", "decr", "plain"]),
    ("lattice10k-rho64-f64-mode2", lambda: lattice_boxes(100, 100, seed=0), "f64", "incidence", 2, dict(rho=64.0), 0, ["plain"] * 6),
    ("lattice10k-f32-mode2", lambda: lattice_boxes(100, 100, seed=0), "f32", "incidence", 2, dict(), 6, ["plain", "incr", "decr", "plain"]),
    ("lattice40x40-edge-major-f64-mode2", lambda: lattice_boxes(40, 40, seed=3), "f64", "edge", 2, dict(), 5, ["plain", "incr", "decr", "plain"]),
    ("lattice520-f64-mode2", ("lattice", 520, 520, 2, 0), "f64", "incidence", 2, dict(), 3, ["plain", "incr", "decr"]),
    ("lattice20x18-partitioned-serial-mode3", lambda: lattice_boxes(20, 18, seed=2), "f64", "incidence", 3, dict(), 6, ["plain", "incr", "plain", "decr", "plain"]),
    ("lattice40x40-partitioned-overlap-mode3", lambda: lattice_boxes(40, 40, seed=3), "f32", "edge", 3, dict(), 6, ["plain", "incr", "plain", "decr", "plain"]),
]
NATURAL = {"benchmark4-rho1/64-mode1": "increase", "benchmark1-rho64-mode1": "decrease", "lattice10k-rho64-f64-mode2": "decrease"}


@pytest.mark.parametrize("entry", FUSED, ids=[f[0] for f in FUSED])
def test_fused_launches_per_iteration(torch_gpu, graphs, entry):
    torch = torch_gpu
    name, graph, dtype, columns, mode, extra, warm, schedule = entry
    if isinstance(graph, tuple):
        g = graphs.get(graph)
        if g is None:
            g = graphs[graph] = lattice_boxes(graph[1], graph[2], n=graph[3], seed=graph[4])
    else:
        g = graph()
    params = dict(tau_incr=3.0, tau_decr=2.0, max_it=60); params.update(extra)
    cp = lr.control_params(tau_incr=3.0, tau_decr=2.0, max_it=60, rho=params.get("rho", 1.0))
    kw = dict(program="wavefront") if mode == 3 else {}
    d, d0 = _handle(g, None, dtype, columns, **kw), _handle(g, None, dtype, columns, **kw)
    if mode == 3:
        d.attach_comm(0, 1, d.unique_id(), {}, {})
        nb = d.set_overlap(1 if "overlap" in name else 2)
        assert (nb > 0) == ("overlap" in name)
    run = d.enqueue_partitioned if mode == 3 else d.enqueue
    assert {1: g.num_edges <= lr.EDGE_BLOCK, 2: g.num_edges > lr.EDGE_BLOCK, 3: True}[mode]       # which kernel mode the launch takes
    tail, head, ic, ec = _layout(d, g, None)
    npdt = np.float64 if dtype == "f64" else np.float32
    nx, nmu = float(g.nx), float(g.nmu)
    crafted = {"incr": INCR, "decr": DECR}
    d.reset(**params)
    run(warm)
    seen, worst, off, scales = set(), 0.0, 0.0, set()
    for k, pre in enumerate(schedule):
        if pre != "plain":
            d.control(torch.tensor(crafted[pre], dtype=torch.float64, device=d.device))
        z0, m0 = d.zedge.clone(), d.mu.clone()
        cb0 = lr.cb_dict(d.read_control()); trace0 = _np(d.trace)
        assert cb0["status"] == lr.RUNNING
        run(1)
        cb1 = lr.cb_dict(d.read_control())
        copy = _np(d.copy)
        what = f"{name} {dtype} MODE {mode} iteration {cb0['it']} mu_scale {cb0['mu_scale']!r}"
        assert np.isfinite(copy).all(), what
        ref = lr.edge_reference(tail, head, copy, _np(z0), _np(m0), cb0["mu_scale"], ic, ec, npdt)
        st = lr.check_edge_step(what, ref, _np(d.zedge), _np(d.mu), cb1["sums"])
        worst = max(worst, st["worst_sum"]); off = max(off, st["mu_off_share"]); scales.add(cb0["mu_scale"])
        assert cb1["inner_failures"] == 0, what
        ref_cb, row, idx = lr.control_reference(cb0, cb1["sums"], cp, nx, nmu, 0, decide_on=cb1)
        lr.check_control(what, ref_cb, row, idx, cb1, trace0, _np(d.trace))
        if cb1["rho"] != cb0["rho"]:
            seen.add("increase" if cb1["rho"] > cb0["rho"] else "decrease")
        # the same edge step in MODE 0 on a second handle: the same bits
        d0.reset(**params)
        if cb0["mu_scale"] != 1.0:
            d0.control(torch.tensor(INCR if cb0["mu_scale"] < 1.0 else DECR, dtype=torch.float64, device=d0.device))
        assert d0.read_control().mu_scale == cb0["mu_scale"]
        d0.zedge.copy_(z0); d0.mu.copy_(m0); d0.copy.copy_(d.copy)
        s0 = _np(d0.edge_step())
        for label, a, b in (("sums", s0, cb1["sums"]), ("zedge", _np(d0.zedge), _np(d.zedge)), ("mu", _np(d0.mu), _np(d.mu))):
            assert _same_bits(a, b), f"{what}: {label} of MODE {mode} differ from MODE 0 at {_first_diff(a, b)}: {a.ravel()[:5]} / {b.ravel()[:5]}"
        if cb1["status"] != lr.RUNNING:
            break
    print(f"LOOPREF fused {name} {dtype} MODE {mode} (E {g.num_edges}): worst sum {worst:.2e} of its bound, largest share of mu words off "
          f"{off:.3e}, mu_scale seen {sorted(scales)}, rho changes inside the fused control step {sorted(seen)}, sums / zedge / mu equal MODE 0 bitwise")
    if name in NATURAL:
        assert NATURAL[name] in seen, f"{name}: the run was to {NATURAL[name]} rho inside a fused control step"
        assert any(s != 1.0 for s in scales), f"{name}: no edge step ran with mu_scale != 1"
    else:
        assert {1.0, 1.0 / 3.0, 3.0} <= scales
    # the ticket is left usable: one iteration twice equals two at once, from the same snapshot
    if mode != 1:
        tensors = (d.copy, d.mu, d.zedge, d.xv, d.zv, d.yv)
        snap = [t.clone() for t in tensors]
        outs = []
        for split in ((1, 1), (2,)):
            for t, s in zip(tensors, snap):
                t.copy_(s)
            d.reset(zero_state=False, **params)
            for n_it in split:
                run(n_it)
            outs.append([_np(t).copy() for t in tensors] + [_np(d.trace)[:2].copy(), np.frombuffer(bytes(d.read_control()), dtype=np.uint8).copy()])
        for a, b in zip(*outs):
            assert _same_bits(a, b), f"{name}: two launches of one iteration differ from one launch of two at {_first_diff(a, b) if a.dtype != np.uint8 else 'the control block'}"
    d.close(); d0.close()


# -------------------------------------------------------------------------------------------------
# (c) the control step alone
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", lr.CONTROL_TABLE, ids=[t[0] for t in lr.CONTROL_TABLE])
def test_control_step_on_crafted_sums(torch_gpu, entry):
    torch = torch_gpu
    from test_loop_reference import EXPECTED_END
    name, p, steps = entry
    g = _fixture_graph("benchmark4")
    d = _handle(g, None, "f64", "incidence")
    d.reset(rho=p["rho"], tau_incr=p["tau_incr"], tau_decr=p["tau_decr"], nu=p["nu"], it_rho_limit=p["it_rho_limit"], max_it=max(p["max_it"], 1),
            eps_abs=p["eps_abs"], eps_rel=p["eps_rel"])
    if d.trace.shape[0] < 8:      # (max_it rows: the gated steps after MAX_IT must still have rows they could wrongly write)
        d.trace = torch.zeros(8, 6, dtype=torch.float64, device=d.device)
    for k, sums in enumerate(steps):
        cb0 = lr.cb_dict(d.read_control()); trace0 = _np(d.trace)
        d.control(torch.tensor(sums, dtype=torch.float64, device=d.device))
        cb1 = lr.cb_dict(d.read_control())
        ref_cb, row, idx = lr.control_reference(cb0, sums, p, float(g.nx), float(g.nmu), 0, decide_on=cb1)
        lr.check_control(f"{name} step {k} (device control_kernel)", ref_cb, row, idx, cb1, trace0, _np(d.trace))
    assert (cb1["rho"], cb1["mu_scale"], cb1["it"], cb1["status"]) == EXPECTED_END[name], name
    d.close()


def test_inner_failures_on_both_loops(torch_gpu):
    """ipm_max_iter = 2: every generic vertex fails its solve.  The count of a step reaches the control block and trace column 5
    on the plain loop (from the handle's counter) and on the partitioned loop (through sums[5] and the all-reduce) alike, and the
    control step clears the counter: a step with no failing solve behind it reports 0."""
    torch = torch_gpu
    g = lattice_boxes(8, 7, seed=3)
    a = _handle(g, None, "f64", "incidence", program="wavefront"); b = _handle(g, None, "f64", "incidence", program="wavefront")
    b.attach_comm(0, 1, b.unique_id(), {}, {})
    counts = []
    for d, run in ((a, a.enqueue), (b, b.enqueue_partitioned)):
        d.reset(max_it=10, ipm_max_iter=2)
        got = []
        for it in range(3):
            run(1)
            cb = d.read_control()
            assert cb.status == lr.RUNNING and cb.it == it + 2
            got.append(cb.inner_failures)
        assert got == [int(x) for x in _np(d.trace)[:3, 5]], got
        counts.append(got)
        d.control(torch.tensor(NEUTRAL, dtype=torch.float64, device=d.device))        # no vertex step behind it
        cb = d.read_control()
        assert cb.inner_failures == 0 and cb.it == 5 and _np(d.trace)[3, 5] == 0.0
    assert counts[0] == counts[1] and min(counts[0]) > 0, counts       # (how many fail: test_inner_failure_keeps_previous_copy)
    a.close(); b.close()


# -------------------------------------------------------------------------------------------------
# (d) the status gate
# -------------------------------------------------------------------------------------------------
def _everything(d):
    return [_np(t).copy() for t in (d.copy, d.mu, d.zedge, d.xv, d.zv, d.yv, d.sums, d.trace)] + \
           [np.frombuffer(bytes(d.read_control()), dtype=np.uint8).copy()]


NAMES = ("copy", "mu", "zedge", "xv", "zv", "yv", "sums", "trace", "control block")


@pytest.mark.parametrize("how", ["converged", "max_it", "diverged", "diverged_partitioned"])
def test_status_gate(torch_gpu, how):
    """after CONVERGED, MAX_IT and DIVERGED every entry point leaves the state, the sums, the control block and the trace as they are.
    (DIVERGED is reached with a NaN the test writes into copy: data, not a fault.)"""
    torch = torch_gpu
    attached = how in ("max_it", "diverged_partitioned")
    if how == "converged":
        d = _handle(_fixture_graph("benchmark4"), None, "f64", "incidence")
        d.solve()
        want = lr.CONVERGED
    else:
        g = lattice_boxes(20, 18, seed=2) if attached else lattice_boxes(40, 40, seed=3)
        d = _handle(g, None, "f64" if how != "diverged" else "f32", "incidence", program="wavefront")
        if attached:
            d.attach_comm(0, 1, d.unique_id(), {}, {})
        run = d.enqueue_partitioned if attached else d.enqueue
        if how == "max_it":
            d.reset(max_it=3)
            run(5)
            want = lr.MAX_IT
        else:
            d.reset(max_it=20)
            run(2)
            d.copy[1, 7] = float("nan")
            d.edge_step(); d.control()
            want = lr.DIVERGED
            assert torch.isnan(d.zedge).any() and lr.cb_dict(d.read_control())["it"] == 3
    assert d.read_control().status == want, (how, d.read_control().status)
    before = _everything(d)
    ops = [("enqueue(3)", lambda: d.enqueue(3)), ("vertex_step", d.vertex_step), ("edge_step", d.edge_step), ("control", d.control),
           ("control(crafted)", lambda: d.control(torch.tensor(INCR, dtype=torch.float64, device=d.device)))]
    if attached:
        ops.append(("enqueue_partitioned(2)", lambda: d.enqueue_partitioned(2)))
    for label, op in ops:
        op()
        for nm, a, b in zip(NAMES, before, _everything(d)):
            assert _same_bits(a, b), f"status gate ({how}): {label} changed {nm}"
    d.close()


# -------------------------------------------------------------------------------------------------
# (e) the cost
# -------------------------------------------------------------------------------------------------
COSTS = [("benchmark4", "f64", None), ("lattice10k", "f64", None), ("lattice10k", "f32", None), ("lattice_n6", "f64", None),
         ("partition", "f64", (1, 2)), ("partition", "f32", (0, 2))]


@pytest.mark.parametrize("name,dtype,part", COSTS, ids=[f"{c[0]}-{c[1]}" for c in COSTS])
def test_cost_of_the_last_iterate(torch_gpu, name, dtype, part):
    g = {"benchmark4": lambda: _fixture_graph("benchmark4"), "lattice10k": lambda: lattice_boxes(100, 100, seed=0),
         "lattice_n6": lambda: lattice_boxes(7, 6, n=6, seed=1), "partition": lambda: lattice_boxes(24, 26, seed=5)}[name]()
    p = None
    if part is not None:
        from gcs_admm_amd.partition import build_partition, strip_owner
        p = build_partition(g, strip_owner(g, part[1]), part[0], part[1])
        g = p.graph
        assert 0 < int(p.edge_counted.sum()) < g.num_edges
    d = _handle(g, p, dtype, "incidence")
    d.reset(max_it=30)
    d.enqueue(10)            # (a partition alone, its ghost columns left at zero: any iterate will do for the cost)
    dev = d.cost()
    zedge = _np(d.zedge)
    ref, abs_terms = lr.cost_reference(_np(d.zv), zedge, g.n, d.params.eps_edge, None if p is None else p.edge_counted)
    frac = lr.check_cost(f"{name} {dtype} cost (V {g.num_vertices}, E {g.num_edges})", ref, abs_terms, dev, g.num_vertices, g.num_edges, g.n)
    assert ref > 0 and np.abs(zedge[2 * g.n]).max() > 0
    print(f"LOOPREF cost {name} {dtype} (V {g.num_vertices}, E {g.num_edges}): {frac:.2e} of its bound")
    d.close()
