"""A batch made with GCSADMM_BATCH_LARGE (gcsadmm_batch_create_ex, ``BatchSolver(..., large=True)``) against the same handles driven
alone.  The statement is test_gpu_batch.py's: a member equals BIT FOR BIT the solo DeviceSolver built with the same knobs and driven
with the same chunking -- status, iteration count, the whole control block, the whole trace, all six state arrays and the cost.  New
ground here: members on the wavefront program (vertex_wave_batch_kernel runs vertex_kernel's body on the member blockIdx.y names), in
every group of instantiations, packed, beside workgroup members, and with more units than a plain batch takes."""
import numpy as np
import pytest

from test_gpu_batch import assert_same, snapshot

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED = -1, 0
WAVE = dict(program="wavefront")
WG = dict(program="workgroup256")


def graph(name):
    from gcs_admm_amd.cases import load_fixture
    from gcs_admm_amd.graph import lattice_boxes
    return lattice_boxes(*name) if isinstance(name, tuple) else load_fixture(name)[1]


def solver(name, dtype="f64", **knobs):
    from gcs_admm_amd.solver import DeviceSolver
    return DeviceSolver(graph(name), dtype, device=0, **knobs)


def solo_shots(name, dtype, knobs, chunks, **params):
    """the graph on a solver of its own: exactly the iterations of ``chunks``, a snapshot after each"""
    d = solver(name, dtype, **knobs)
    d.reset(**params)
    shots = []
    for k in chunks:
        d.enqueue(k)
        shots.append(snapshot(d))
    d.close()
    return shots


def solo_to_end(name, dtype, knobs, chunk=25, **params):
    d = solver(name, dtype, **knobs)
    d.reset(**params)
    done = 0
    while True:
        d.enqueue(chunk)
        done += chunk
        if d.read_control().status != RUNNING or done >= d.params.max_it:
            break
    out = snapshot(d)
    d.close()
    return out


def large_batch(members, dtype="f64"):
    """BatchSolver.of over new solvers: members = [(graph name, knobs)]"""
    from gcs_admm_amd import BatchSolver
    return BatchSolver.of([solver(n, dtype, **k) for n, k in members], large=True)


def close(batch):
    batch.close()
    for m in batch.members:
        m.close()


def check_chunks(members, chunks, dtype="f64", params=None):
    """the batch and every solo driven through ``chunks``: equal after every chunk"""
    batch = large_batch(members, dtype)
    batch.reset(params)
    want = [solo_shots(n, dtype, k, chunks, **(params[i] if params else {})) for i, (n, k) in enumerate(members)]
    for c, k in enumerate(chunks):
        batch.enqueue(k)
        for i, (n, _) in enumerate(members):
            assert_same(snapshot(batch.members[i]), want[i][c], (n, dtype, "after chunk", c))
    return batch


def test_wavefront_solo_runs_repeat_bit_for_bit():
    """the precondition of every comparison below: two solo runs of benchmark1 on the wavefront program leave identical traces and state"""
    a, b = solo_to_end("benchmark1", "f64", WAVE), solo_to_end("benchmark1", "f64", WAVE)
    assert_same(a, b, "benchmark1 on the wavefront program, two solo runs")
    assert a["status"] == CONVERGED


FOUR = ["test1", "benchmark1", "benchmark2", "benchmark4"]


def test_generic_members_to_their_stops():
    """the generic instantiation, grids of 1, 4 and 39 wavefronts in one launch, f64 to every member's stop test; benchmark1 stops
    before benchmark2, and from the poll that first reports it stopped its state does not change"""
    batch = large_batch([(n, WAVE) for n in FOUR])
    assert batch.launches() == (0, 1, 4)
    batch.reset()
    early, done = {}, 0
    while True:
        batch.enqueue(5)
        done += 5
        status, it = batch.poll()
        if status[1] != RUNNING and not early:
            early["b1"] = snapshot(batch.members[1], cost=False)
            early["b2_running"] = status[2] == RUNNING
        if all(s != RUNNING for s in status) or done >= 1000:
            break
    assert early and early["b2_running"]
    assert_same(snapshot(batch.members[1], cost=False), early["b1"], "benchmark1 after its stop")
    for i, n in enumerate(FOUR):
        want = solo_to_end(n, "f64", WAVE, chunk=5)
        assert_same(snapshot(batch.members[i]), want, n)
        assert want["status"] == CONVERGED
    close(batch)


def test_generic_members_f32():
    close(check_chunks([(n, WAVE) for n in FOUR], [30], "f32"))


def test_box_members_and_a_two_block_edge_step():
    """the box instantiation: 3 x 3, 5 x 4 and 12 x 12 lattices (9, 20, 144 wavefronts; the last has two edge workgroups) after 1, 2
    and 30 iterations, and enqueued one iteration at a time"""
    members = [((3, 3), WAVE), ((5, 4), WAVE), ((12, 12), WAVE)]
    batch = check_chunks(members, [1, 1, 28])
    assert batch.launches() == (0, 1, 3)
    close(batch)
    close(check_chunks(members, [1] * 30))


def test_several_groups_in_one_batch():
    """12 x 12 aligned, dense, without stored dual directions and on generic rows, plus benchmark1 aligned and dense: every
    instantiation choice in one batch.  The generic-rows lattice and the aligned benchmark1 choose the same instantiation (generic,
    aligned, stored directions) and so share a launch: the plan's rule -- one launch per (all_m4, align_rows, store_dl) -- gives four
    launches for those five members; the dense benchmark1 is the fifth."""
    members = [((12, 12), WAVE), ((12, 12), dict(WAVE, wave_align=2)), ((12, 12), dict(WAVE, wave_store_dl=2)),
               ((12, 12), dict(WAVE, wave_generic_rows=1)), ("benchmark1", WAVE)]
    batch = check_chunks(members, [20])
    assert batch.launches() == (0, 4, 5)
    close(batch)
    batch = check_chunks(members + [("benchmark1", dict(WAVE, wave_align=2))], [20])
    assert batch.launches() == (0, 5, 6)
    close(batch)


def test_packed_members():
    """four vertices per wavefront: two 12 x 12 members against solos packed the same way"""
    close(check_chunks([((12, 12), dict(WAVE, wave_slots=4))] * 2, [1, 19]))


def test_no_reorder_in_the_batch():
    """1 000 wavefronts: the solo handle reorders its dispatch slowest-first every 8 iterations, the batch never does -- the same bits
    after 1, 9 and 30 iterations, beside a small member"""
    close(check_chunks([((25, 40), WAVE), ((5, 4), WAVE)], [1, 8, 21]))


def test_mixed_batch_and_more_than_512_workgroup_vertices():
    """a wavefront member, a workgroup member and the 24 x 24 workgroup member a plain batch refuses (576 vertices)"""
    batch = check_chunks([((12, 12), WAVE), ("benchmark4", WG), ((24, 24), WG)], [20])
    assert batch.launches() == (2, 1, 1)
    close(batch)


def test_one_member_with_both_kinds_of_vertices():
    """512 vertices of degree 66 on the workgroup program and a chain of 12 on the wavefront program in one handle (the graph of
    test_batch_large_plan.mixed_graph): a row of the workgroup launch and a row of a wave launch, which carries its closed-form
    vertices, beside a wavefront member and a workgroup member"""
    from gcs_admm_amd import BatchSolver
    from gcs_admm_amd.solver import DeviceSolver
    from test_batch_large_plan import mixed_graph
    g = mixed_graph()
    mixed = lambda: DeviceSolver(g, "f64", device=0, **WAVE)
    d = mixed()
    q = d.query()
    assert q["num_workgroup_vertices"] == 512 and q["num_waves"] == 12, q
    d.reset()
    want = []
    for k in (1, 9):
        d.enqueue(k)
        want.append(snapshot(d))
    d.close()
    batch = BatchSolver.of([solver((5, 4), **WAVE), mixed(), solver("benchmark4", **WG)], large=True)
    assert batch.launches() == (2, 1, 2)
    batch.reset()
    for c, k in enumerate((1, 9)):
        batch.enqueue(k)
        assert_same(snapshot(batch.members[1]), want[c], ("mixed member after chunk", c))
    assert np.all(np.isfinite(want[-1]["trace"][:10]))
    close(batch)


def test_every_member_has_its_own_parameters():
    params = [dict(rho=1.0), dict(rho=4.0, cold_start=True), dict(rho=0.25)]
    batch = check_chunks([("benchmark1", WAVE)] * 3, [25, 25], params=params)
    assert len({snapshot(m)["trace"].tobytes() for m in batch.members}) == 3      # the members did run differently
    close(batch)


def test_plain_batch_still_refuses_a_wavefront_member():
    from gcs_admm_amd import BatchSolver
    from gcs_admm_amd.abi import GcsAdmmError
    d = solver("benchmark1", **WAVE)
    with pytest.raises(GcsAdmmError, match=r"member 0: vertices on the wavefront program \(create the handle with vertex_program = 3\)"):
        BatchSolver.of([d], large=False)
    with pytest.raises(GcsAdmmError, match=r"member 0: vertices on the wavefront program"):
        BatchSolver.of([d])
    d.close()


def _lattice_sets(nx, ny):
    """the cells of ``lattice_boxes(nx, ny)`` as regions by key: the scene of tools/prune_bench.py"""
    g = graph((nx, ny))
    cells = range(2, g.num_vertices)
    return ({("cell", v - 2): g.poly_A[g.poly_ptr[v]:g.poly_ptr[v + 1]] for v in cells},
            {("cell", v - 2): g.poly_b[g.poly_ptr[v]:g.poly_ptr[v + 1]] for v in cells})


def test_scene_queries_end_to_end():
    """two local queries on the 25 x 40 brick lattice: unpruned, each query graph has 1 000 generic vertices, which a plain batch
    refuses and ``large=True`` solves; every record is the solo DeviceSolver of that graph under the member's knobs.  Pruned to their
    informed sets the graphs are small, and ``large=True`` takes the path ``large=False`` takes."""
    from gcs_admm_amd.abi import GcsAdmmError
    from gcs_admm_amd.batch import member_programs
    from gcs_admm_amd.queries import SceneQueries
    from gcs_admm_amd.solver import DeviceSolver
    nx, ny, common = 25, 40, dict(max_it=300)
    with SceneQueries(*_lattice_sets(nx, ny), 2) as sq:
        cell = lambda i, j: j * nx + i
        a, b = [cell(3, 5), cell(17, 30)], [cell(5, 8), cell(19, 33)]
        S, G = sq.centers[a], sq.centers[b]
        with pytest.raises(GcsAdmmError, match="member 0: 512 or more workgroup-program vertices"):
            sq.solve(S, G, **common)
        records = sq.solve(S, G, large=True, return_state=True, **common)
        assert len(records) == 2
        knobs = member_programs([r["graph"] for r in records], large=True)
        assert knobs == [dict(program="wavefront", wave_slots=2)] * 2
        for rec, k in zip(records, knobs):
            d = DeviceSolver(rec["graph"], "f64", device=0, **k)
            want = d.solve(chunk=25, **common)
            assert rec["iterations"] == want["iterations"] > 0 and rec["status"] == want["status"]
            assert np.float64(rec["cost"]).tobytes() == np.float64(want["cost"]).tobytes()
            assert rec["trace"].tobytes() == d.trace.cpu().numpy().tobytes()
            for f, v in rec["state"].items():
                assert v.tobytes() == getattr(d, f).cpu().numpy().tobytes(), f
            assert np.isfinite(rec["rounded_cost"])
            d.close()
        small, plain = (sq.solve(S, G, prune="informed", large=flag, return_state=True, **common) for flag in (True, False))
        for x, y in zip(small, plain):
            assert x["kept_regions"] == y["kept_regions"] < 512
            assert (x["iterations"], x["status"], x["rounded_cost"]) == (y["iterations"], y["status"], y["rounded_cost"])
            assert np.float64(x["cost"]).tobytes() == np.float64(y["cost"]).tobytes() and x["trace"].tobytes() == y["trace"].tobytes()
            for f in x["state"]:
                assert x["state"][f].tobytes() == y["state"][f].tobytes(), f
