"""The candidate rule of the rounding step, held to the sequential host loop on every entry point: ``rounding`` with both
restrictions, ``rounding_many`` and ``rounding_members`` visit the paths that loop visits, in its order, and return its result bit
for bit.  The yardstick is that loop as it stood when every entry point had a copy of its own, with the path solve injected and the
result rule of the batched entries (a solve without a finite cost is never the result) at its end.  Small random digraphs, a fake
solver that decides from a checksum of the path; no GPU, no native build."""
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from gcs_admm_amd import rounding as R

n = 2
GRAPHS = 40
NS, MS, SEEDS = (0, 1, 2, 5), (0, 1, 3, 20), (0, 1, 2)


def digraph(g):
    """'s', 3 to 8 inner vertices, 't'; every ordered pair an edge with probability 0.5, none into 's' or out of 't'; activations
    uniform in (0, 1), 15 % of them exactly 0"""
    rng = np.random.default_rng(1000 + g)
    V = ['s'] + list(range(int(rng.integers(3, 9)))) + ['t']
    E = [(u, v) for u in V for v in V if u != v and v != 's' and u != 't' and rng.random() < 0.5]
    y_e = {e: 0.0 if rng.random() < 0.15 else float(1.0 - rng.random()) for e in E}
    I_out = {v: [e for e in E if e[0] == v] for v in V}
    return V, E, y_e, I_out


def fake_solve(path, salt, failing):
    """a third of the paths infeasible; with ``failing`` a further seventh failed (cost inf WITH a point); else a finite cost"""
    h = zlib.crc32(repr((tuple(path), salt)).encode())
    if h % 3 == 0:
        return float('inf'), None
    xs = {v: np.full(2 * n, (h % 1009) / 16.0 + j) for j, v in enumerate(path)}
    if failing and (h // 3) % 7 == 0:
        return float('inf'), xs
    return 1.0 + (h // 21) % 997 / 8.0, xs


def yardstick(y_e_sol, V, I_v_out, N, M, seed, solve):
    """the sequential host loop; returns (visited paths, draws taken, (cost, x_v, y_v))"""
    visited, draws = [], 0

    def solve_path_restriction(path):
        visited.append(tuple(path))
        return solve(path)
    rng = np.random.default_rng(seed)
    seen, cands = set(), []
    first = R.most_probable_path(y_e_sol, I_v_out)
    if first is not None:
        seen.add(tuple(first))
        cost, xs = solve_path_restriction(first)
        if xs is not None:
            cands.append((cost, first, xs))
    for _ in range(M):
        if len(cands) >= N:
            break
        draws += 1
        pth = R.find_path_via_random_dfs(y_e_sol, I_v_out, rng)
        if pth is None or tuple(pth) in seen:
            continue
        seen.add(tuple(pth))
        cost, xs = solve_path_restriction(pth)
        if xs is not None:
            cands.append((cost, pth, xs))
    cands = [c for c in cands if np.isfinite(c[0])]
    if not cands:
        return visited, draws, (float('inf'), None, None)
    cost, pth, xs = min(cands, key=lambda t: t[0])
    return visited, draws, (cost, {v: xs.get(v, np.zeros(2 * n)) for v in V}, {v: (1 if v in xs else 0) for v in V})


def assert_same_result(got, want, what):
    (c, x, y), (cw, xw, yw) = got, want
    assert np.float64(c).tobytes() == np.float64(cw).tobytes(), what
    if xw is None:
        assert x is None and y is None, what
        return
    assert y == yw and list(y) == list(yw) and list(x) == list(xw), what
    assert all(np.asarray(x[v]).tobytes() == np.asarray(xw[v]).tobytes() for v in xw), what


def eager_sampler(problems, calls):
    """the sampler of ``rounding_members`` on the host's draws, all of them drawn up front: walk 0 the most probable path, walks
    1 .. count - 1 from one generator per member; vertex indices, status 0 or 1"""
    def sample(members, graphs, seeds, count):
        calls.append(count)
        out = []
        for (V, y_e, I_out), seed in zip(problems, seeds):
            rng = np.random.default_rng(seed)
            walks = [R.most_probable_path(y_e, I_out)] + [R.find_path_via_random_dfs(y_e, I_out, rng) for _ in range(count - 1)]
            out.append(([np.array([V.index(v) for v in (w or ['s'])], np.int32) for w in walks], np.array([w is None for w in walks], np.int32)))
        return out
    return sample


@pytest.mark.parametrize("failing", [False, True], ids=["plain", "failed_solves"])
@pytest.mark.parametrize("g", range(GRAPHS))
def test_every_entry_point_follows_the_host_loop(g, failing, monkeypatch):
    V, E, y_e, I_out = digraph(g)
    As = {v: np.zeros((1, n)) for v in V}
    bs = {v: np.zeros(1) for v in V}
    graph = SimpleNamespace(n=n, keys=V, poly_ptr=np.arange(len(V) + 1), poly_A=np.zeros((len(V), n)), poly_b=np.zeros(len(V)))
    salt = g
    draws = []
    walk = R.find_path_via_random_dfs

    def counted_walk(*a):
        draws[-1] += 1
        return walk(*a)
    monkeypatch.setattr(R, "find_path_via_random_dfs", counted_walk)
    for N in NS:
        for M in MS:
            alone = {}
            for seed in SEEDS:
                what = (g, N, M, seed)
                draws.append(0)
                want_visited, want_draws, want = yardstick(y_e, V, I_out, N, M, seed, lambda p: fake_solve(p, salt, failing))
                draws[-1] = 0                       # (the yardstick draws through the module too)
                if not failing:                     # 1. the host restriction
                    seen = []

                    def fake_host(As_, bs_, n_, path):
                        assert As_ is As and bs_ is bs and n_ == n
                        seen.append(tuple(path))
                        return fake_solve(path, salt, False)
                    monkeypatch.setattr(R, "solve_path_restriction", fake_host)
                    got = R.rounding(y_e, V, E, I_out, As, bs, n, N=N, M=M, seed=seed)
                    assert seen == want_visited and draws[-1] == want_draws, what
                    assert_same_result(got, want, what)
                seen, calls = [], []

                def fake_dev(As_, bs_, n_, paths):    # 2. the round loop on an injected solver
                    assert As_ is As and bs_ is bs and n_ == n and len(paths) >= 1
                    calls.append(len(paths)); seen.extend(tuple(p) for p in paths)
                    return [fake_solve(p, salt, failing) for p in paths]
                draws.append(0)
                got = R.rounding(y_e, V, E, I_out, As, bs, n, N=N, M=M, seed=seed, restriction="device", solver=fake_dev)
                assert seen == want_visited and draws[-1] == want_draws, what
                assert_same_result(got, want, what)
                alone[seed] = (want_visited, got)
            log = []

            def fake_many(As_, bs_, n_, paths):
                assert n_ == n and set(As_) == set(bs_) == {(i, v) for i in range(len(SEEDS)) for v in V}
                assert all(len({i for i, _ in p}) == 1 and p[0][0] == p[-1][0] for p in paths)
                log.extend((p[0][0], tuple(v for _, v in p)) for p in paths)
                out = []
                for p in paths:
                    cost, xs = fake_solve([v for _, v in p], salt, failing)
                    out.append((cost, None if xs is None else {(p[0][0], v): x for v, x in xs.items()}))
                return out
            # 3. many problems, one call per round
            draws.append(0)
            problems = [dict(y_e_sol=y_e, V=V, E=E, I_v_out=I_out, As=As, bs=bs, n=n, seed=seed) for seed in SEEDS]
            many = R.rounding_many(problems, N=N, M=M, solver=fake_many)
            for i, seed in enumerate(SEEDS):
                assert [p for j, p in log if j == i] == alone[seed][0], (g, N, M, seed)
                assert_same_result(many[i], alone[seed][1], (g, N, M, seed, "many"))
            # 4. the same walks, drawn up front
            del log[:]
            sampled = []
            members = R.rounding_members([None] * len(SEEDS), [graph] * len(SEEDS), N=N, M=M, seeds=list(SEEDS),
                                         sampler=eager_sampler([(V, y_e, I_out)] * len(SEEDS), sampled), solver=fake_many)
            assert sampled == [M + 1]
            for i, seed in enumerate(SEEDS):
                assert [p for j, p in log if j == i] == alone[seed][0], (g, N, M, seed)
                assert_same_result(members[i], alone[seed][1], (g, N, M, seed, "members"))


def test_the_cases_reach_every_branch_of_the_accounting():
    """over the 40 graphs: a missing walk 0, dead ends, duplicates, a later round after an infeasible one, failed solves that hold a
    slot, and problems in which nothing is feasible"""
    no_first = dead = dup = later = held = nothing = 0
    for g in range(GRAPHS):
        V, E, y_e, I_out = digraph(g)
        no_first += R.most_probable_path(y_e, I_out) is None
        rng = np.random.default_rng(0)
        walks = [R.find_path_via_random_dfs(y_e, I_out, rng) for _ in range(20)]
        dead += sum(w is None for w in walks)
        live = [tuple(w) for w in walks if w is not None]
        dup += len(live) - len(set(live))
        rounds = []
        out = R.rounding(y_e, V, E, I_out, None, None, n, N=2, M=20, restriction="device",
                         solver=lambda As_, bs_, n_, paths: rounds.append(paths) or [fake_solve(p, g, True) for p in paths])
        later += len(rounds) >= 2
        held += any(xs is not None and not np.isfinite(cost) for rnd in rounds for cost, xs in (fake_solve(p, g, True) for p in rnd))
        nothing += out[1] is None
    assert min(no_first, dead, dup, later, held, nothing) >= 1, (no_first, dead, dup, later, held, nothing)
