"""The state transfer on the device: state_export_kernel and state_import_kernel through the C ABI on the tables of
state_transfer_cases.py against ``transfer_reference``, bit for bit (test_state_transfer.py runs the same tables through the host
build); the batch calls against solo calls, in plain, ``large`` and ``region_terminals`` batches; and replanning end to end on
benchmark4's regions: ``SceneQueries.solve(keep=True)``, then ``solve(seed=...)`` on the moved query, which must stop in at most half
the iterations of the same query from zero at the same rounded cost -- unpruned and pruned, and across an ``add_regions`` and a
``remove_regions``.  A ``solve`` without ``keep`` and ``seed`` is what it was: its trace and state against a batch driven by hand."""
import numpy as np
import pytest

import locate_cases as L
import replanning_cases as R
import state_transfer_cases as X

pytestmark = pytest.mark.gpu

WG = dict(program="workgroup256")


def member(s, **knobs):
    """a DeviceSolver of the Side's graph, reset at its rho, holding its state"""
    import torch
    from gcs_admm_amd.solver import DeviceSolver
    m = DeviceSolver(s.g, s.dtype, device=0, columns=s.columns, **{**WG, **knobs})
    m.reset(rho=s.rho)
    load(m, s.state)
    return m


def load(m, state):
    import torch
    for k in X.STATE:
        getattr(m, k).copy_(torch.from_numpy(state[k]))


def read(m):
    return {k: getattr(m, k).cpu().numpy() for k in X.STATE}


def snapshot_read(snap):
    return dict(snap.arrays(), V=snap.V, E=snap.E)


def transfer(src, dst, **knobs):
    """export ``src``, import into ``dst`` on the device, one solo call each: (the snapshot's arrays, dst's state after)"""
    a, b = member(src, **knobs), member(dst, **knobs)
    try:
        snap = a.export_state(src.ids)
        b.import_state(snap, dst.ids)
        return snapshot_read(snap), read(b)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("label,s", list(X.round_trip_cases()), ids=[l for l, _ in X.round_trip_cases()])
def test_export_then_import_is_the_identity(label, s):
    snap, state = transfer(s, X.Side(s.g, s.ids, s.columns, s.dtype, fill="nan"))
    X.same_snapshot(snap, X.export_reference(s), label)
    X.same_state(state, s.state, label)


@pytest.mark.parametrize("dtype,columns", [("f64", ("incidence", "edge")), ("f32", ("edge", "incidence"))])
def test_different_graphs_equal_the_reference(dtype, columns):
    seen = 0
    for label, src, dst in list(X.pair_cases(dtype=dtype, columns=columns)) + list(X.neighbour_key_cases(dtype=dtype)):
        snap, state = transfer(src, dst)
        X.same_snapshot(snap, X.export_reference(src), label)
        X.same_state(state, X.transfer_reference(src, dst), label)
        seen += 1
    assert seen >= 2 * len(X.SIZES) + 11


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rho_scales_mu_alone(dtype):
    """a source at rho 4.5 into a member at rho 1 (the pending mu_scale of a control block cannot be set through the ABI: the host
    build holds that half)"""
    src = X.side(2, 65, dtype=dtype, rho=4.5, seed=4)
    dst = X.Side(src.g, src.ids, "edge", dtype, fill="nan", rho=1.0)
    snap, state = transfer(src, dst)
    assert snap["rho"][0] == 4.5
    X.same_state(state, X.transfer_reference(src, dst))
    E, T = src.g.num_edges, X.NP_DTYPE[dtype]
    assert state["mu"][:, :E].tobytes() == np.ascontiguousarray((src.state["mu"][:, src.tail_col].astype(np.float64) * 4.5).astype(T)).tobytes()


# ------------------------------------------------------------------------------------------- batches
def batch_round(sources, dests, skip=(), knobs=None, **flags):
    """export the sources in one batch call, import into the destinations in another (``skip``: members handed a null snapshot);
    (the snapshots' arrays or None, the destinations' states after)"""
    from gcs_admm_amd import BatchSolver
    knobs = knobs or [{}] * len(sources)
    src_m = [member(s, **k) for s, k in zip(sources, knobs)]
    dst_m = [member(d, **k) for d, k in zip(dests, knobs)]
    a, b = BatchSolver.of(src_m, **flags), BatchSolver.of(dst_m, **flags)
    try:
        a.reset(params=[dict(rho=s.rho) for s in sources]); b.reset(params=[dict(rho=d.rho) for d in dests])
        for m, s in zip(src_m + dst_m, list(sources) + list(dests)):      # (reset zeroes the state)
            load(m, s.state)
        snaps = a.export_state([s.ids for s in sources])
        seed = [None if k in skip else s for k, s in enumerate(snaps)]
        b.import_state(seed, [d.ids for d in dests])
        return [snapshot_read(s) for s in snaps], [read(m) for m in dst_m]
    finally:
        a.close(); b.close()
        for m in src_m + dst_m:
            m.close()


def test_a_batch_with_a_null_snapshot_equals_the_solo_calls():
    sources = [X.side(2, E, columns=("incidence", "edge")[k % 2], seed=k) for k, E in enumerate((5, 257, 64, 1, 300))]
    dests = [X.subgraph_side(s, np.arange(s.g.num_vertices) % 4 != 3, columns=("edge", "incidence")[k % 2], fill="nan") for k, s in enumerate(sources)]
    snaps, states = batch_round(sources, dests, skip=(2,))
    for k, (s, d) in enumerate(zip(sources, dests)):
        X.same_snapshot(snaps[k], X.export_reference(s), k)
        if k == 2:
            X.same_state(states[k], d.state, k)                      # not touched
            continue
        solo_snap, solo_state = transfer(s, d)
        X.same_state(states[k], solo_state, k)
        X.same_state(states[k], X.transfer_reference(s, d), k)
        X.same_snapshot(snaps[k], solo_snap, k)


def _sides_of(graphs, dtype="f64"):
    ids = [np.concatenate([[0, 1], 2 + 3 * np.arange(g.num_vertices - 2)]) for g in graphs]
    return ([X.Side(g, i, "incidence", dtype, seed=k) for k, (g, i) in enumerate(zip(graphs, ids))],
            [X.Side(g, i, "incidence", dtype, fill="nan") for g, i in zip(graphs, ids)])


def test_a_large_batch_of_wavefront_members():
    from gcs_admm_amd.graph import lattice_boxes
    sources, dests = _sides_of([lattice_boxes(5, 4), lattice_boxes(3, 3), lattice_boxes(12, 12)])
    snaps, states = batch_round(sources, dests, knobs=[dict(program="wavefront")] * 3, large=True)
    for k, (s, d) in enumerate(zip(sources, dests)):
        X.same_snapshot(snaps[k], X.export_reference(s), k)
        X.same_state(states[k], X.transfer_reference(s, d), k)


def test_a_batch_with_region_terminals():
    import batch_terminals_cases as bc
    sources, dests = _sides_of([bc.graph(name) for name in ("row", "scene1", "scene2")])
    snaps, states = batch_round(sources, dests, region_terminals=True)
    for k, (s, d) in enumerate(zip(sources, dests)):
        X.same_snapshot(snaps[k], X.export_reference(s), k)
        X.same_state(states[k], X.transfer_reference(s, d), k)


def test_refusals_reach_the_caller_and_write_nothing():
    from gcs_admm_amd.abi import GcsAdmmError
    s = X.side(2, 20, seed=6)
    m = member(X.Side(s.g, s.ids, fill="nan"))
    try:
        snap = member(s)
        good = snap.export_state(s.ids)
        snap.close()
        with pytest.raises(ValueError, match="ascend strictly"):
            m.import_state(good, s.ids[::-1])
        bad = X.Side(X.graph_of(2, 5, [2, 3, 2], [3, 4, 4]), [0, 1, 2, 3, 4])
        u = member(bad)
        with pytest.raises(GcsAdmmError, match="not strictly ascending in"):
            u.export_state(bad.ids)
        u.close()
        f32 = member(X.Side(s.g, s.ids, dtype="f32"))
        with pytest.raises(GcsAdmmError, match="n or state_dtype"):
            f32.import_state(good, s.ids)
        f32.close()
        assert all(np.isnan(a).all() for a in read(m).values())
    finally:
        m.close()


# ------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def scene():
    from gcs_admm_amd import SceneQueries
    As, bs, n, _ = L.region_sets(R.NAME)
    ref = R.Scene()
    with SceneQueries(As, bs, n, device=0) as sq:
        yield sq, ref.s[None], ref.t[None], As, bs


def _meets_the_claim(cold, seeded, label):
    print(label, "cold", cold["iterations"], "seeded", seeded["iterations"], "rounded", cold["rounded_cost"], seeded["rounded_cost"])
    assert cold["status"] == seeded["status"] == "converged", label
    assert 2 * seeded["iterations"] <= cold["iterations"], (label, seeded["iterations"], cold["iterations"])
    assert abs(seeded["rounded_cost"] - cold["rounded_cost"]) <= 1e-5, (label, seeded["rounded_cost"], cold["rounded_cost"])


@pytest.mark.parametrize("how", [dict(), dict(prune="informed", assemble="induced")], ids=["whole", "pruned"])
def test_a_seeded_solve_stops_in_half_the_iterations(scene, how):
    sq, S, G, _, _ = scene
    base, = sq.solve(S, G, keep=True, **how)
    assert base["snapshot"].V == base["graph"].num_vertices and base["snapshot"].E == base["graph"].num_edges
    moved = S + 0.2 * np.asarray(R.DIRECTION)
    cold, = sq.solve(moved, G, **how)
    seeded, = sq.solve(moved, G, seed=[base["snapshot"]], **how)
    _meets_the_claim(cold, seeded, how)
    base["snapshot"].close()


def test_a_seed_survives_add_and_remove_regions(scene):
    sq, S, G, As, bs = scene
    base, = sq.solve(S, G, keep=True, return_state=True)
    quiet = [k for k, y in zip(base["graph"].keys, base["state"]["yv"]) if k not in ('s', 't') and y < R.NO_FLOW]
    assert quiet
    gone = quiet[0]
    box = np.vstack([np.eye(2), -np.eye(2)])
    extra = {"added": box}, {"added": np.array([40.0, 40.0, -39.0, -39.0])}      # a region far from everything
    try:
        sq.add_regions(*extra)
        sq.remove_regions([gone])
        moved = S + 0.2 * np.asarray(R.DIRECTION)
        cold, = sq.solve(moved, G)
        seeded, = sq.solve(moved, G, seed=[base["snapshot"]])
        assert gone not in cold["graph"].keys and "added" in cold["graph"].keys
        assert sq.vertex_ids(cold["graph"])[-1] == len(As) + 2
        _meets_the_claim(cold, seeded, "edited")
    finally:
        base["snapshot"].close()
        sq.remove_regions(["added"])
        sq.add_regions({gone: As[gone]}, {gone: bs[gone]})


def test_without_seed_and_keep_solve_is_a_batch_driven_by_hand(scene):
    from gcs_admm_amd import BatchSolver
    sq, S, G, _, _ = scene
    starts, goals = np.vstack([S, S + 0.2 * np.asarray(R.DIRECTION)]), np.vstack([G, G])
    recs = sq.solve(starts, goals, return_state=True)
    batch = BatchSolver(sq.graphs(starts, goals), "f64", device=0)
    try:
        hand = batch.solve()
        for r, h, m in zip(recs, hand, batch.members):
            assert "snapshot" not in r
            assert (r["iterations"], r["status"], r["cost"]) == (h["iterations"], h["status"], h["cost"])
            assert r["trace"].tobytes() == m.trace.cpu().numpy().tobytes()
            X.same_state(r["state"], read(m))
    finally:
        batch.close()
        for m in batch.members:
            m.close()
