"""A batch of handles (gcsadmm_batch_*, gcs_admm_amd/batch.py) against the same handles driven alone.  The batch kernels run the device
functions of the solo kernels on each member's own arguments and control state, so the statement is equality BIT FOR BIT: status,
iteration count, the whole control block, the whole trace, every state array and the cost.  "Solo" is a
DeviceSolver(program="workgroup256") of the same graph and state type, driven by ``enqueue`` with the same chunking.  The oracle is
not needed: solo handles are held to it by test_gpu_parity.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED = -1, 0
STATE = ("copy", "mu", "zedge", "xv", "zv", "yv")


def _graph(name):
    from gcs_admm_amd.cases import load_fixture
    from gcs_admm_amd.graph import lattice_boxes
    if isinstance(name, tuple):
        nx, ny, n, seed = name
        return lattice_boxes(nx, ny, n=n, seed=seed)
    return load_fixture(name)[1]


def snapshot(d, cost=True):
    """everything a run leaves behind on one solver, as host bytes"""
    cb = d.read_control()
    out = dict(status=cb.status, it=cb.it, cb=bytes(cb), trace=d.trace.cpu().numpy().copy())
    for k in STATE:
        out[k] = getattr(d, k).cpu().numpy().copy()
    if cost:
        out["cost"] = d.cost()
    return out


def assert_same(a, b, what):
    assert (a["status"], a["it"]) == (b["status"], b["it"]), what
    assert a["cb"] == b["cb"], (what, "control block")
    for k in ("trace",) + STATE:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float(np.nanmax(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)))))
    if "cost" in a and "cost" in b:
        assert np.float64(a["cost"]).tobytes() == np.float64(b["cost"]).tobytes(), (what, "cost", a["cost"], b["cost"])


def solo_run(name, dtype="f64", chunks=None, chunk=25, **params):
    """the graph on a solver of its own: to its stop test in chunks of ``chunk``, or exactly the iterations of ``chunks`` with a snapshot
    after each; returns the final snapshot (or the list of them)"""
    from gcs_admm_amd.solver import DeviceSolver
    d = DeviceSolver(_graph(name), dtype, device=0, program="workgroup256")
    d.reset(**params)
    if chunks is not None:
        shots = []
        for k in chunks:
            d.enqueue(k)
            shots.append(snapshot(d))
        d.close()
        return shots
    done = 0
    while True:
        d.enqueue(chunk)
        done += chunk
        if d.read_control().status != RUNNING or done >= d.params.max_it:
            break
    out = snapshot(d)
    d.close()
    return out


_solo_cache = {}


def solo(name, dtype="f64"):
    """default-parameter solo run to the end, computed once per (graph, state type) and shared by the tests"""
    if (name, dtype) not in _solo_cache:
        _solo_cache[(name, dtype)] = solo_run(name, dtype)
    return _solo_cache[(name, dtype)]


def batch_to_end(batch, chunk=25, on_poll=None):
    done, max_it = 0, max(m.params.max_it for m in batch.members)
    while True:
        batch.enqueue(chunk)
        done += chunk
        status, it = batch.poll()
        if on_poll:
            on_poll(status, it)
        if all(s != RUNNING for s in status) or done >= max_it:
            return status, it


FOUR = ["test1", "test2", "benchmark1", "benchmark2"]


def test_solo_runs_repeat_bit_for_bit():
    """the precondition of every comparison below: two solo runs of benchmark1 leave identical traces and final state"""
    a, b = solo("benchmark1"), solo_run("benchmark1")
    assert_same(a, b, "benchmark1, two solo runs")
    assert a["status"] == CONVERGED and a["it"] == 39


@pytest.mark.parametrize("dtype,names", [("f64", FOUR), ("f32", ["test1", "benchmark1"])])
def test_members_equal_their_solo_runs(dtype, names):
    """default parameters, to the end: every member of the batch is its solo run; the stop iterations are the reference records'"""
    from gcs_admm_amd import BatchSolver
    batch = BatchSolver([_graph(n) for n in names], dtype, device=0)
    res = batch.solve(chunk=25)
    status, it = batch.poll()
    for i, n in enumerate(names):
        got, want = snapshot(batch.members[i]), solo(n, dtype)
        assert_same(got, want, (n, dtype))
        assert (status[i], it[i]) == (want["status"], want["it"]) and res[i]["iterations"] == want["it"] and res[i]["cost"] == want["cost"]
    if dtype == "f64":
        from gcs_admm_amd.cases import load_fixture
        assert it[2] == 39 == load_fixture("benchmark1")[0]["golden_v3"]["iterations"]
        assert it[3] == 100 == load_fixture("benchmark2")[0]["golden_v3"]["iterations"]
        assert status[2] == status[3] == CONVERGED
    batch.close()


def test_a_member_that_stops_is_left_alone():
    """benchmark1 converges at 39 while benchmark2 runs to 100: from the poll that first reports it CONVERGED to the end of the batch its
    state, control block and trace do not change, and the slowest member still arrives at its solo iterate"""
    from gcs_admm_amd import BatchSolver
    batch = BatchSolver([_graph(n) for n in FOUR], "f64", device=0)
    batch.reset()
    early = {}

    def on_poll(status, it):
        if status[2] == CONVERGED and not early:
            early["b1"] = snapshot(batch.members[2], cost=False)
            early["others_running"] = status[3] == RUNNING
    batch_to_end(batch, chunk=5, on_poll=on_poll)
    assert early and early["others_running"]
    assert_same(snapshot(batch.members[2], cost=False), early["b1"], "benchmark1 after its stop")
    for i, n in enumerate(FOUR):
        assert_same(snapshot(batch.members[i]), solo(n), n)
    batch.close()


def test_every_member_has_its_own_parameters():
    from gcs_admm_amd import BatchSolver
    params = [dict(rho=1.0, tau_incr=3.0), dict(rho=4.0, cold_start=True), dict(rho=0.25)]
    batch = BatchSolver([_graph("benchmark1")] * 3, "f64", device=0)
    batch.solve(chunk=25, params=params)
    shots = [snapshot(m) for m in batch.members]
    for i, p in enumerate(params):
        assert_same(shots[i], solo_run("benchmark1", **p), p)
    assert len({s["trace"].tobytes() for s in shots}) == 3      # the members did run differently
    batch.close()


def test_multi_block_edge_step_and_uneven_grids():
    """test1 (1 vertex workgroup, 1 edge workgroup), a 12 x 12 lattice (144 and 2: the ticket hand-off) and benchmark4 in one batch:
    bit-identical to solo after 1, 2 and 30 iterations (the ticket is reset and reused), and 30 calls of enqueue(1) equal one enqueue(30)"""
    from gcs_admm_amd import BatchSolver
    names = ["test1", (12, 12, 2, 0), "benchmark4"]
    chunks = [1, 1, 28]
    want = [solo_run(n, chunks=chunks) for n in names]
    batch = BatchSolver([_graph(n) for n in names], "f64", device=0)
    assert _graph(names[1]).num_edges > 256
    # (edge_blocks of the lattice member is 2: pinned on the host by test_batch_plan.py; here by its grid)
    assert -(-_graph(names[1]).num_edges // 256) > 1
    batch.reset()
    for c, k in enumerate(chunks):
        batch.enqueue(k)
        for i, n in enumerate(names):
            assert_same(snapshot(batch.members[i]), want[i][c], (n, "after", sum(chunks[:c + 1])))
    batch.reset()
    for _ in range(30):
        batch.enqueue(1)
    for i, n in enumerate(names):
        assert_same(snapshot(batch.members[i]), want[i][-1], (n, "30 x enqueue(1)"))
    batch.close()


@pytest.mark.parametrize("shape", [[(5, 5, 3, s) for s in range(3)], [(4, 4, 6, s) for s in range(2)]], ids=["n3", "n6"])
def test_box_instantiation_and_other_dimensions(shape):
    """box lattices at n = 3 and n = 6 run the BOX instantiation of the batch kernel (47 KB of LDS per workgroup at n = 6: three per CU)"""
    from gcs_admm_amd import BatchSolver
    batch = BatchSolver([_graph(n) for n in shape], "f64", device=0)
    batch.reset()
    batch.enqueue(20)
    for i, n in enumerate(shape):
        got = snapshot(batch.members[i])
        assert_same(got, solo_run(n, chunks=[20])[0], n)
        assert got["it"] > 1 and np.isfinite(got["trace"][:got["it"] - 1]).all()
    batch.close()


def test_refusals_on_the_device_path():
    from gcs_admm_amd import BatchSolver
    from gcs_admm_amd.abi import GcsAdmmError
    from gcs_admm_amd.solver import DeviceSolver
    mk = lambda name: DeviceSolver(_graph(name), "f64", device=0, program="workgroup256")
    a, b, c = mk("benchmark1"), mk("test1"), mk("benchmark1")
    with pytest.raises(GcsAdmmError, match="at least one member"):
        BatchSolver.of([])
    with pytest.raises(GcsAdmmError, match="member 1: the handle appears twice"):
        BatchSolver.of([a, a])
    # bind before reset
    batch = BatchSolver.of([a, b])
    with pytest.raises(GcsAdmmError, match="member 0: gcsadmm_reset has not been called"):
        batch.bind()
    with pytest.raises(GcsAdmmError, match="gcsadmm_batch_bind has not been called"):
        batch.enqueue(1)
    batch.reset()
    # a member of a batch that is bound cannot be bound by another one ...
    other = BatchSolver.of([b, c])
    c.reset()
    with pytest.raises(GcsAdmmError, match="member 0: the handle is bound to another batch"):
        other.bind()
    # ... and a reset of a member behind the batch's back is noticed
    a.reset(rho=2.0)
    with pytest.raises(GcsAdmmError, match="member 0: gcsadmm_reset was called after gcsadmm_batch_bind"):
        batch.enqueue(1)
    # a communicator attached after the batch was made: refused at bind
    c.attach_comm(0, 1, None, {}, {})
    with pytest.raises(GcsAdmmError, match="member 1: a communicator is attached"):
        other.bind()
    with pytest.raises(GcsAdmmError, match="member 0: a communicator is attached"):
        BatchSolver.of([c])
    # once the batch is destroyed its members are free: for the other batch (without the partitioned handle) and on their own
    batch.close()
    other.close()
    again = BatchSolver.of([b])
    again.solve()
    assert_same(snapshot(b), solo("test1"), "test1 in a second batch")
    again.close()
    a.solve()
    assert_same(snapshot(a), solo("benchmark1"), "benchmark1 alone after its batch was destroyed")
    # a member destroyed before its batch leaves it: the batch refuses to be bound and can still be destroyed
    orphan = BatchSolver.of([a, b])
    b.close()
    with pytest.raises(GcsAdmmError, match="member 1: null handle"):
        orphan.bind()
    orphan.close()
    for d in (a, c):
        d.close()


def test_a_stopped_batch_changes_nothing():
    """with every member stopped, gcsadmm_batch_run enqueues kernels that leave at once: no state, control block or trace changes"""
    from gcs_admm_amd import BatchSolver
    names = ["test1", "benchmark1"]
    batch = BatchSolver([_graph(n) for n in names], "f64", device=0)
    batch.solve()
    before = [snapshot(m) for m in batch.members]
    assert all(s["status"] != RUNNING for s in before)
    batch.enqueue(5)
    status, it = batch.poll()
    for i, n in enumerate(names):
        assert_same(snapshot(batch.members[i]), before[i], n)
        assert (status[i], it[i]) == (before[i]["status"], before[i]["it"])
    batch.close()
