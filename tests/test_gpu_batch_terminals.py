"""A batch made with GCSADMM_BATCH_TERMINALS (BatchSolver(region_terminals=True)) against the same handles driven alone.  The batch's
terminal kernel runs the device function of the solo kernel on each terminal's own arguments, workspace and warm-start records, so
the statement is the one of test_gpu_batch.py: equality BIT FOR BIT of status, iteration count, the whole control block, the whole
trace, all six state arrays and the cost.  "Solo" is a DeviceSolver of the same graph with the same knobs, driven by ``enqueue`` with
the same chunking; solo handles with region terminals are held to the oracle by test_gpu_configs.py and test_gpu_scaled_steps.py.
The members are those of test_batch_terminals_plan.py (batch_terminals_cases.py), which pins the launches they make."""
import numpy as np
import pytest

import batch_terminals_cases as bc
from test_gpu_batch import RUNNING, assert_same, batch_to_end, snapshot

pytestmark = pytest.mark.gpu

WG = dict(program="workgroup256")
N2 = ["row", "scene1", "scene2", "star2x33"]         # (64, LDS) x 6 terminals and (256, LDS) x 1: two launches per iteration
REGION_TEXT = "a terminal that is a region"


def solver(name, dtype="f64", **knobs):
    from gcs_admm_amd.solver import DeviceSolver
    return DeviceSolver(bc.graph(name), dtype, device=0, **{**WG, **knobs})


def solo_run(name, dtype="f64", chunks=None, chunk=25, knobs=None, **params):
    """the graph on a solver of its own: to its stop test in chunks of ``chunk``, or exactly the iterations of ``chunks`` with a snapshot
    after each; the final snapshot (or the list of them)"""
    d = solver(name, dtype, **(knobs or {}))
    d.reset(**params)
    shots, done = [], 0
    if chunks is not None:
        for k in chunks:
            d.enqueue(k)
            shots.append(snapshot(d))
        d.close()
        return shots
    while True:
        d.enqueue(chunk)
        done += chunk
        if d.read_control().status != RUNNING or done >= d.params.max_it:
            break
    out = snapshot(d)
    d.close()
    return out


_solo = {}


def solo(name, dtype="f64"):
    """default-parameter solo run to the end, once per (graph, state type)"""
    if (name, dtype) not in _solo:
        _solo[(name, dtype)] = solo_run(name, dtype)
    return _solo[(name, dtype)]


def batch_of(names, dtype="f64", **kw):
    from gcs_admm_amd import BatchSolver
    return BatchSolver([bc.graph(k) for k in names], dtype, device=0, region_terminals=True, **kw)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_members_equal_their_solo_runs(dtype):
    """default parameters, to the stop: every member is its solo run, the 64-thread and the 256-thread launch side by side"""
    batch = batch_of(N2, dtype)
    assert batch.terminal_launches() == (2, 7) and batch.launches() == (4, 0, 0)
    res = batch.solve(chunk=25)
    status, it = batch.poll()
    for i, k in enumerate(N2):
        want = solo(k, dtype)
        assert_same(snapshot(batch.members[i]), want, (k, dtype))
        assert (status[i], it[i]) == (want["status"], want["it"]) and res[i]["cost"] == want["cost"]
        assert want["it"] > 1
    batch.close()


@pytest.mark.parametrize("names,launches", [(["star3", "star3b"], (1, 2)), (["star8", "star8b"], (1, 2)), (["star6"], (1, 1)),
                                            (["star6", "simplex6"], (2, 2))], ids=["n3", "n8", "n6", "n6 both workspace groups"])
def test_in_chunks_at_other_dimensions(names, launches):
    """n = 3 and n = 8 (one wavefront, LDS), n = 6 with 30 live edges (256 threads, the handle's workspace) and beside it the simplex
    source (one wavefront, workspace): bit-identical to solo after 1, 2 and 12 iterations"""
    chunks = [1, 1, 10]
    batch = batch_of(names)
    assert batch.terminal_launches() == launches
    batch.reset()
    want = [solo_run(k, chunks=chunks) for k in names]
    for c, n_it in enumerate(chunks):
        batch.enqueue(n_it)
        for i, k in enumerate(names):
            got = snapshot(batch.members[i])
            assert_same(got, want[i][c], (k, "after", sum(chunks[:c + 1])))
    assert all(w[-1]["it"] > 2 for w in want)
    batch.close()


def test_cold_start_on_one_member_only():
    """``cold_start`` lives in the parameters: the bind gives that member's terminals no warm-start records and the others theirs"""
    names = ["scene1", "row", "scene2"]
    params = [dict(), dict(cold_start=True, rho=2.0), dict(rho=0.5)]
    batch = batch_of(names)
    batch.solve(chunk=25, params=params)
    for i, (k, p) in enumerate(zip(names, params)):
        assert_same(snapshot(batch.members[i]), solo_run(k, **p), (k, p))
    batch.close()


def test_a_member_that_stops_is_left_alone():
    """from the poll that first finds a member stopped while another runs on, that member's state, control block and trace do not
    change (its terminal workgroups leave at once), and every member still arrives at its solo iterate"""
    batch = batch_of(N2)
    batch.reset()
    early = {}

    def on_poll(status, it):
        if not early and any(s != RUNNING for s in status) and any(s == RUNNING for s in status):
            early["who"] = [i for i, s in enumerate(status) if s != RUNNING]
            early["shots"] = [snapshot(batch.members[i], cost=False) for i in early["who"]]
    batch_to_end(batch, chunk=5, on_poll=on_poll)
    assert early, "no member stopped before the others: choose other members"
    for i, shot in zip(early["who"], early["shots"]):
        assert_same(snapshot(batch.members[i], cost=False), shot, (N2[i], "after its stop"))
    for i, k in enumerate(N2):
        assert_same(snapshot(batch.members[i]), solo(k), k)
    batch.close()


def test_with_batch_large_a_wavefront_member_has_region_terminals():
    """GCSADMM_BATCH_LARGE | GCSADMM_BATCH_TERMINALS: region_scene(1) on the wavefront program beside the row on the workgroup program"""
    from gcs_admm_amd import BatchSolver
    knobs = [dict(program="wavefront"), WG]
    names = ["scene1", "row"]
    members = [solver(k, **kn) for k, kn in zip(names, knobs)]
    batch = BatchSolver.of(members, large=True, region_terminals=True)
    assert batch.launches() == (1, 1, 1) and batch.terminal_launches() == (1, 4)
    batch.solve(chunk=25)
    for i, (k, kn) in enumerate(zip(names, knobs)):
        got = snapshot(members[i])
        assert_same(got, solo_run(k, knobs=kn), (k, kn))
        assert got["it"] > 1
    batch.close()
    for m in members:
        m.close()


def test_without_the_flag_the_refusal_stands():
    """a plain batch and a GCSADMM_BATCH_LARGE batch refuse the member as before; members without region terminals make no terminal launch"""
    from gcs_admm_amd import BatchSolver
    from gcs_admm_amd.abi import GcsAdmmError
    from gcs_admm_amd.cases import load_fixture
    row = solver("row")
    for kw in (dict(), dict(large=True)):
        with pytest.raises(GcsAdmmError, match="member 0: " + REGION_TEXT):
            BatchSolver.of([row], **kw)
    plain = BatchSolver([load_fixture("test1")[1]], "f64", device=0, region_terminals=True)
    assert plain.terminal_launches() == (0, 0)
    plain.close()
    row.close()


# ------------------------------------------------------------------------------------------- end to end: SceneQueries with box terminals
def _in_polytope(A, b, x, slack=1e-7):
    return bool(np.all(np.asarray(A) @ x <= np.asarray(b) + slack))


def _ordered_path(rec, n):
    """the vertices of the rounded path from 's' to 't', by the shared end points of their segments"""
    x, y = rec["x_v_rounded"], rec["y_v_rounded"]
    on = [v for v in rec["graph"].keys if y[v] == 1]
    path, left = ['s'], [v for v in on if v != 's']
    while path[-1] != 't':
        nxt = [v for v in left if np.allclose(np.asarray(x[v])[:n], np.asarray(x[path[-1]])[n:], rtol=0, atol=1e-9)]
        assert nxt, (path, left)
        path.append(nxt[0]); left.remove(nxt[0])
    assert not left
    return path


def test_scene_query_between_two_boxes_finds_the_known_answer():
    """the row of region_row as a scene of ONE region with start_boxes = [0,1]^2 and goal_boxes = [2,3] x [0,1]: the graph is
    region_row's, the run converges to its known cost (length 1 between the faces x = 1 and x = 2, + 2 edges x 1e-4; the bound of
    test_region_terminals_whole_run), and the rounded cost is the host restriction's on the same sets and path"""
    from gcs_admm_amd import SceneQueries
    from gcs_admm_amd.graph import sets_of_graph
    from gcs_admm_amd.rounding import solve_path_restriction
    from test_path_restrict import path_bound
    row = bc.graph("row")
    As_row, bs_row = sets_of_graph(row)
    sb = (np.array([[0.0, 0.0]]), np.array([[1.0, 1.0]])); gb = (np.array([[2.0, 0.0]]), np.array([[3.0, 1.0]]))
    with SceneQueries({0: As_row[0]}, {0: bs_row[0]}, 2) as sq:
        for assemble in ("host", "device"):
            (g,) = sq.graphs(start_boxes=sb, goal_boxes=gb, assemble=assemble)
            for f in ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr", "poly_A", "poly_b"):
                a, b = getattr(g, f), getattr(row, f)
                # (region_row writes its bounds from integers: its -lo is 0.0 where the box [hi; -lo] of a float lo = 0 has -0.0)
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (assemble, f)
            # the terminals' interiors are the boxes' centres; the region's is the scene's centre LP, the host's to its tolerance
            assert g.interior[:2].tobytes() == row.interior[:2].tobytes() and np.allclose(g.interior[2], row.interior[2], rtol=0, atol=1e-6)
        (rec,) = sq.solve(start_boxes=sb, goal_boxes=gb)
    print("relaxed cost", rec["cost"], "rounded cost", rec["rounded_cost"], "iterations", rec["iterations"])
    assert rec["status"] == "converged"
    assert abs(rec["cost"] - 1.0002) < 1e-2
    path = _ordered_path(rec, 2)
    assert path == ['s', 0, 't']
    As, bs = sets_of_graph(rec["graph"])
    host, _ = solve_path_restriction(As, bs, 2, path)
    print("host restriction", host)
    assert abs(rec["rounded_cost"] - host) <= 2.0 * (path_bound(As, path) + 1e-12 * max(1.0, host))
    assert abs(host - 1.0) < 1e-6


def _lattice_queries():
    """(As, bs of the 36 cells of a 6 x 6 lattice, 8 start points, 8 goal boxes): starts at cell centres, goals boxes of half-widths
    0.1 .. 0.45 about other cells' centres -- inside one cell up to across its neighbours"""
    from gcs_admm_amd.graph import lattice_boxes, sets_of_graph
    As, bs = sets_of_graph(lattice_boxes(6, 6))
    As = {k: np.array(v) for k, v in As.items() if k not in ('s', 't')}; bs = {k: np.array(v) for k, v in bs.items() if k not in ('s', 't')}
    cen = {k: 0.5 * (bs[k][:2] - bs[k][2:]) for k in As}
    rng = np.random.default_rng(6)
    a, b = rng.permutation(36)[:8], rng.permutation(36)[:8]
    S = np.array([cen[int(k)] for k in a]) + rng.uniform(-0.1, 0.1, (8, 2))
    c = np.array([cen[int(k)] for k in b]); h = rng.uniform(0.1, 0.45, (8, 2))
    return As, bs, S, (c - h, c + h)


_lattice = {}


def lattice_solos():
    """the graphs of the 8 lattice queries and, per graph, the result and snapshot of a solo DeviceSolver, computed once"""
    if not _lattice:
        from gcs_admm_amd import SceneQueries
        from gcs_admm_amd.solver import DeviceSolver
        As, bs, S, gb = _lattice_queries()
        with SceneQueries(As, bs, 2) as sq:
            graphs = sq.graphs(starts=S, goal_boxes=gb)
        solos = []
        for g in graphs:
            d = DeviceSolver(g, "f64", device=0, program="workgroup256")
            res = d.solve()
            solos.append((res, snapshot(d)))
            d.close()
        _lattice.update(graphs=graphs, solos=solos)
    return _lattice["graphs"], _lattice["solos"]


@pytest.mark.parametrize("walk", ["host", "device"])
def test_lattice_queries_with_point_starts_and_box_goals(walk):
    """8 queries on a 6 x 6 lattice scene in one batch made with region_terminals: every record's relaxed solve is a solo DeviceSolver
    on the same graph bit for bit, and every rounded path starts in the start's box, ends in the goal box and keeps consecutive points
    in a common region, to 1e-7"""
    from gcs_admm_amd import SceneQueries
    from gcs_admm_amd.graph import sets_of_graph
    As, bs, S, gb = _lattice_queries()
    graphs, solos = lattice_solos()
    with SceneQueries(As, bs, 2) as sq:
        records = sq.solve(starts=S, goal_boxes=gb, walk=walk, return_state=True, assemble="device" if walk == "device" else "host")
    assert len(records) == 8
    for i, (rec, (want, shot)) in enumerate(zip(records, solos)):
        assert rec["graph"].edge_tail.tobytes() == graphs[i].edge_tail.tobytes() and rec["graph"].poly_b.tobytes() == graphs[i].poly_b.tobytes()
        assert (rec["status"], rec["iterations"]) == (want["status"], want["iterations"]), i
        assert rec["trace"].tobytes() == shot["trace"].tobytes(), (i, "trace")
        for k, a in rec["state"].items():
            assert a.tobytes() == shot[k].tobytes(), (i, k)
        assert np.float64(rec["cost"]).tobytes() == np.float64(want["cost"]).tobytes()
        assert np.isfinite(rec["rounded_cost"]), i
        x = rec["x_v_rounded"]
        sets_A, sets_b = sets_of_graph(rec["graph"])
        path = _ordered_path(rec, 2)
        first, last = np.asarray(x['s'])[:2], np.asarray(x['t'])[2:]
        assert np.all(np.abs(first - S[i]) <= 1e-6 + 1e-7), (i, first, S[i])
        assert np.all(last >= gb[0][i] - 1e-7) and np.all(last <= gb[1][i] + 1e-7), (i, last)
        for v in path:
            for half in (np.asarray(x[v])[:2], np.asarray(x[v])[2:]):
                assert _in_polytope(sets_A[v], sets_b[v], half), (i, v)
