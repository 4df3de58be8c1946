"""The device walk of the rounding step without a GPU: the host build of walk_kernel (tests/hostemu/walk_emu.cpp on
csrc/path_walk_core.h, the 64 lanes one after the other) against the rule's Python restatement ``walks.walk_reference`` element for
element; the rule itself (what it does case by case, its draw frequencies, walk 0 against the host's most probable path); and
``rounding_members`` on an injected sampler and solver.  The same cases run on the device in test_gpu_path_walk.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import restrict_cases as R
import walk_cases as WC
from gcs_admm_amd import walks as W
from gcs_admm_amd.rounding import most_probable_path, rounding_members, solve_path_restriction


# ------------------------------------------------------------------------------------------- the pieces
def test_weight_mix_and_mulhi_of_the_host_build():
    lib = WC.emu()
    ys = [2.0 ** -41, 2.0 ** -40, np.nextafter(2.0 ** -40, 0), 1.0, 1.0000001, 1.9999999, 2.0, 5.0, np.inf, 0.0, -0.0, -0.1, -np.inf, np.nan,
          5e-324, float(np.float32(0.3)), 0.3]
    want = [0, 1, 0, 2 ** 40, int(np.floor(1.0000001 * 2.0 ** 40)), int(np.floor(1.9999999 * 2.0 ** 40)), 2 ** 41, 2 ** 41, 2 ** 41, 0, 0, 0, 0, 0, 0,
            int(np.floor(float(np.float32(0.3)) * 2.0 ** 40)), int(np.floor(0.3 * 2.0 ** 40))]
    assert [W.weight(y) for y in ys] == want
    assert [lib.walk_emu_weight(y) for y in ys] == want
    # splitmix64: the first outputs of the generator seeded with 0 are those of the counters 1, 2, 3 (Vigna's reference values)
    assert [W.mix(0, 0, j) for j in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    rng = np.random.default_rng(0)
    for seed, walk, j in [(0, 0, 0), (7, 1, 0), (2 ** 63 + 5, 20, 41), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 2)] + \
            [(int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32 - 1))) for _ in range(50)]:
        assert lib.walk_emu_mix(seed, walk, j) == W.mix(seed, walk, j), (seed, walk, j)
    for a, b in [(2 ** 64 - 1, 2 ** 63), (2 ** 64 - 1, 2 ** 64 - 1), (0, 5), (12345678901234567, 2 ** 41 * 130)]:
        assert lib.walk_emu_mulhi(a, b) == (a * b) >> 64


def test_out_lists_are_the_out_dicts_of_rounding_problem():
    from gcs_admm_amd.cases import load_fixture
    g = load_fixture("benchmark3")[1]
    out_ptr, out_head, out_edge = W.out_lists(g)
    E = g.edges_as_keys()
    for v, key in enumerate(g.keys):
        ks = range(out_ptr[v], out_ptr[v + 1])
        assert [E[out_edge[k]] for k in ks] == [e for e in E if e[0] == key]
        assert [g.keys[out_head[k]] for k in ks] == [e[1] for e in E if e[0] == key]
    assert out_ptr[-1] == g.num_edges and out_ptr.dtype == out_head.dtype == out_edge.dtype == np.int32


# ------------------------------------------------------------------------------------------- the rule, case by case
def test_the_rule_on_the_handmade_cases():
    cases = {c.name: c for c in WC.handmade()}
    ref = lambda name, walk, seed=0, dtype=np.float64: WC.reference(cases[name], dtype, seed, walk)
    for walk in range(WC.WALKS):
        path, status = ref("excluded", walk)
        assert (path.tolist(), status) in (([0, 1, 2], W.DEAD_END), ([0, 3], W.OK))
        assert ref("all_zero", walk)[1] == W.DEAD_END and ref("all_zero", walk)[0].tolist() == [0]
        path, status = ref("weights", walk)                  # 2^-41, the negative and the NaN are absent; 2^-40 has weight 1 of 2^40 (2 + ...)
        assert status == W.OK and path[1] in (2, 3, 4, 5) and path.tolist() == [0, path[1], 8]
        assert ref("src_is_dst", walk)[0].tolist() == [0] and ref("src_is_dst", walk)[1] == W.OK
        assert ref("long_chain", walk)[0].tolist() == [0, 1, 2, 3, 4] and ref("long_chain", walk)[1] == W.TOO_LONG
        assert ref("exact_fit", walk)[0].tolist() == list(range(10)) and ref("exact_fit", walk)[1] == W.OK
    assert {ref("excluded", w)[1] for w in range(WC.WALKS)} == {W.OK, W.DEAD_END}
    assert ref("excluded", 0)[0].tolist() == [0, 1, 2]       # walk 0 follows the largest activation into the dead end
    assert ref("weights", 0)[0].tolist() == [0, 5, 8]        # 5.0 is capped at 2, still the largest
    assert ref("tie", 0)[0].tolist() == [0, 2, 3]            # equal weights: the last in out-list order
    star = cases["star130"]
    assert ref("star130", 0)[0].tolist() == [0, 1 + int(np.argmax(star.y[:130])), 131]
    assert len({tuple(ref("star130", w)[0]) for w in range(WC.WALKS)}) > 10


def test_walk_0_is_the_hosts_most_probable_path(oracle_lib):
    """and walks 0 .. 20 give several distinct successful paths on every benchmark"""
    for name in WC.BENCHMARKS:
        b = WC.benchmark(oracle_lib, name)
        g = b.graph
        I_out = {v: [e for e in b.y_e if e[0] == v] for v in g.keys}
        path, status = WC.reference(b, np.float64, 0, 0)
        assert status == W.OK and [g.keys[v] for v in path] == most_probable_path(b.y_e, I_out), name
        ok = {tuple(WC.reference(b, np.float64, 0, w)[0]) for w in range(WC.WALKS) if WC.reference(b, np.float64, 0, w)[1] == W.OK}
        assert len(ok) >= 2, name


@pytest.mark.parametrize("which", ["fan5", "star130"])
def test_draw_frequencies(which):
    """first-step picks of walks 1 .. 4096: every bin within 5 sqrt(W p (1 - p)) of W p, p from the integer weights"""
    case = {c.name: c for c in WC.handmade()}[which]
    draws = 4096
    d = case.out_ptr[1] - case.out_ptr[0]
    w = np.array([W.weight(case.y[case.out_edge[k]]) for k in range(d)], float)
    p = w / w.sum()
    picks = [W.walk_reference(case.out_ptr, case.out_head, case.out_edge, case.y, case.src, case.dst, 0, walk, 2) for walk in range(1, draws + 1)]
    assert all(s == W.TOO_LONG and len(path) == 2 for path, s in picks)
    count = np.bincount([path[1] - 1 for path, _ in picks], minlength=d)          # heads are 1 .. d in out-list order
    dev = np.abs(count - draws * p) / np.sqrt(draws * p * (1 - p))
    print(which, "worst bin", dev.max())
    assert np.all(dev <= 5.0), dev.max()


# ------------------------------------------------------------------------------------------- the host build against the mirror
@pytest.mark.parametrize("dtype", WC.DTYPES, ids=["f64", "f32"])
def test_host_build_equals_the_mirror(oracle_lib, dtype):
    for case in WC.all_cases(oracle_lib):
        for seed in WC.SEEDS:
            rc, paths, status = WC.emu_sample(case, dtype, seed, 0, WC.WALKS)
            assert rc == 0
            WC.assert_equals_reference(case, dtype, seed, 0, paths, status)
        # walks are independent: a later window by itself
        rc, paths, status = WC.emu_sample(case, dtype, 7, 8, 8)
        WC.assert_equals_reference(case, dtype, 7, 8, paths, status)


def test_host_build_checks_the_problem():
    c = {c.name: c for c in WC.handmade()}["excluded"]
    lib = WC.emu()
    out = np.zeros(8, np.int32)

    def rc(V=c.V, out_ptr=c.out_ptr, out_head=c.out_head, out_edge=c.out_edge, src=c.src, dst=c.dst):
        return lib.walk_emu_sample(V, len(out_head), out_ptr.ctypes.data, out_head.ctypes.data, out_edge.ctypes.data, c.y.ctypes.data, 0, src, dst, 0, 0, 1,
                                   4, out.ctypes.data, out[4:].ctypes.data, out[5:].ctypes.data)
    assert rc() == 0
    head = c.out_head.copy(); head[2] = 4
    edge = c.out_edge.copy(); edge[0] = -1
    ptr = c.out_ptr.copy(); ptr[1], ptr[2] = ptr[2], ptr[1]
    assert ptr[1] > ptr[2]
    assert rc(out_head=head) == 1 and rc(out_edge=edge) == 1 and rc(out_ptr=ptr) == 1 and rc(src=4) == 1 and rc(dst=-1) == 1
    assert rc(V=W.MAX_VERTICES + 1) == 2                   # refused before anything of the problem is read


def test_the_largest_out_degree_keeps_the_total_in_64_bits():
    """2^22 entries of the largest weight 2^41: tot = 2^63, r = z >> 1 and the pick is entry z >> 42, exactly; one more entry is refused"""
    V, D = W.MAX_VERTICES, W.MAX_DEGREE
    span = V - 2
    for degree, want_rc in ((D, 0), (D + 1, 2)):
        out_ptr = np.full(V + 1, degree, np.int32); out_ptr[0] = 0
        case = SimpleNamespace(name=f"degree{degree}", V=V, out_ptr=out_ptr, out_head=(1 + np.arange(degree) % span).astype(np.int32),
                               out_edge=np.arange(degree, dtype=np.int32), y=np.full(degree, 7.5), src=0, dst=V - 1, max_len=3)
        rc, paths, status = WC.emu_sample(case, np.float64, 7, 0, 3)
        assert rc == want_rc
        if rc == 0:
            picks = [D - 1] + [W.mix(7, w, 0) >> 42 for w in (1, 2)]
            assert [p.tolist() for p in paths] == [[0, 1 + k % span] for k in picks] and status.tolist() == [W.DEAD_END] * 3


# ------------------------------------------------------------------------------------------- rounding_members, no GPU
def host_solver(log):
    def solve(As, bs, n, paths):
        log.append([list(p) for p in paths])
        return [solve_path_restriction(As, bs, n, p) for p in paths]
    return solve


def expected_candidates(drawn, feasible, N, M):
    """the host loop's accounting, one path after the other: walk 0, then draws 1 .. M while fewer than N paths are feasible"""
    paths, status = drawn
    seen, offered, good = set(), [], 0
    for w in range(M + 1):
        if w > 0 and good >= N:
            break
        if status[w] != W.OK or tuple(paths[w]) in seen:
            continue
        seen.add(tuple(paths[w])); offered.append(list(paths[w]))
        good += feasible(paths[w])
    return offered


def test_rounding_members_on_the_benchmarks(oracle_lib):
    """all four benchmarks as the members of one call: the candidates are the distinct successful walks in walk order, capped by N,
    and the rounded cost is the reference record's"""
    bench = [WC.benchmark(oracle_lib, name) for name in WC.BENCHMARKS]
    graphs = [b.graph for b in bench]
    members = [SimpleNamespace(zedge=np.vstack([np.zeros((2 * b.graph.n, len(b.y))), b.y])) for b in bench]
    seeds = [0, 0, 0, 0]
    log, calls = [], []

    def sampler(*args):
        calls.append(args[3])
        return WC.mirror_sampler(*args)
    out = rounding_members(members, graphs, seeds=seeds, sampler=sampler, solver=host_solver(log))
    assert calls == [21]                                                         # ONE sampler call, walks 0 .. M
    drawn = WC.mirror_sampler(members, graphs, seeds, 21)
    for i, (b, (cost, x_v, y_v)) in enumerate(zip(bench, out)):
        g = b.graph
        offered = [[v for _, v in p] for rnd in log for p in rnd if p[0][0] == i]
        assert all(p[0][0] == p[-1][0] for rnd in log for p in rnd)
        want = expected_candidates(([[g.keys[v] for v in p] for p in drawn[i][0]], drawn[i][1]), lambda p: True, 5, 20)
        assert offered == want and 1 <= len(offered) <= 5, (b.name, offered, want)
        print(b.name, "candidates", len(offered), "cost", cost, "record", R.RECORDS[b.name])
        assert abs(cost - R.RECORDS[b.name]) <= 1e-5 * R.RECORDS[b.name], (b.name, cost)
        assert set(x_v) == set(y_v) == set(g.keys) and y_v['s'] == 1 and y_v['t'] == 1
        best = min((solve_path_restriction(*_sets(g), g.n, p) for p in offered), key=lambda t: t[0])
        assert cost == best[0] and {v for v in g.keys if y_v[v]} == set(best[1])


def _sets(g):
    from gcs_admm_amd.graph import sets_of_graph
    return sets_of_graph(g)


def test_rounding_members_goes_on_drawing_after_an_infeasible_round(oracle_lib):
    """a solver that finds the first two candidates of member 0 infeasible: their places are taken by later draws, in further rounds;
    a member without a successful walk gives (inf, None, None) and does not hold up the others"""
    b = WC.benchmark(oracle_lib, "benchmark3")
    g = b.graph
    row = lambda y: np.vstack([np.zeros((2 * g.n, len(y))), y])
    members = [SimpleNamespace(zedge=row(b.y)), SimpleNamespace(zedge=row(np.zeros_like(b.y))), SimpleNamespace(zedge=row(b.y))]
    graphs, seeds, N, M = [g, g, g], [3, 3, 11], 3, 20
    drawn = WC.mirror_sampler(members, graphs, seeds, M + 1)
    keyed = lambda i: ([[g.keys[v] for v in p] for p in drawn[i][0]], drawn[i][1])
    distinct = expected_candidates(keyed(0), lambda p: True, 99, M)
    assert len(distinct) >= N + 2, len(distinct)
    bad = {tuple(distinct[0]), tuple(distinct[1])}
    log = []

    def solver(As, bs, n, paths):
        log.append([list(p) for p in paths])
        return [(float('inf'), None) if p[0][0] == 0 and tuple(v for _, v in p) in bad else (float(len(p)) + 0.001 * j, {v: np.ones(2 * n) for v in p})
                for j, p in enumerate(paths)]
    out = rounding_members(members, graphs, N=N, M=M, seeds=seeds, sampler=WC.mirror_sampler, solver=solver)
    assert len(log) >= 2
    offered = lambda i: [[v for _, v in p] for rnd in log for p in rnd if p[0][0] == i]
    assert offered(0) == expected_candidates(keyed(0), lambda p: tuple(p) not in bad, N, M) == distinct[:N + 2]
    assert offered(1) == [] and out[1] == (float('inf'), None, None)
    assert offered(2) == expected_candidates(keyed(2), lambda p: True, N, M) and len(offered(2)) == N
    assert len(log[0]) == 2 * N and all(p[0][0] == 0 for rnd in log[1:] for p in rnd)      # the first round: N pending per live member
    cost, x_v, y_v = out[0]
    assert np.isfinite(cost) and {v for v in g.keys if y_v[v]} not in [set(p) for p in bad]
    assert all(np.array_equal(x_v[v], np.ones(4) if y_v[v] else np.zeros(4)) for v in g.keys)


def test_rounding_members_refuses_mismatched_arguments(oracle_lib):
    g = WC.benchmark(oracle_lib, "benchmark1").graph
    with pytest.raises(ValueError, match="one graph per member"):
        rounding_members([None], [g, g], sampler=WC.mirror_sampler, solver=lambda *a: [])
    with pytest.raises(ValueError, match="one seed per member"):
        rounding_members([None], [g], seeds=[1, 2], sampler=WC.mirror_sampler, solver=lambda *a: [])
    assert rounding_members([], [], sampler=None, solver=None) == []


def test_solve_refuses_an_unknown_walk():
    import locate_cases as L
    from gcs_admm_amd.queries import SceneQueries
    As, bs, n, pairs = L.region_sets("four_boxes")
    scene = L.EmuScene([(np.asarray(As[k], float), np.asarray(bs[k], float)) for k in As], pairs)
    with SceneQueries(As, bs, n, scene=scene, pair_lp=L.PairLP()) as sq:
        with pytest.raises(ValueError, match="walk must be 'host' or 'device'"):
            sq.solve([[0.5, 0.5]], [[2.5, 0.5]], walk="bogus")
