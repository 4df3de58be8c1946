"""Cases, bounds and the host emulation for the path-restriction solve (csrc/path_restrict_core.h), shared by test_path_restrict.py
(CPU: the emulation) and test_gpu_path_restrict.py (gcsadmm_scene_restrict_paths).  A solver here is any callable
``solve(n, polys, paths, starts, tol, max_iter) -> (points per path, cost, iterations, status)`` on region INDICES.

Exact answers (boxes of half-width 0.6 on unit-spaced centres, the ends are regions): a corridor of k boxes along e_0 costs
(k - 1) - 1.2; a staircase of 2K + 1 boxes costs sqrt(2) (K - 1.2) and half of its segments have length zero; the elbow costs 1.6;
the all-zero case costs 0.  Bound on |cost - exact|: 2 deg tol + 1e-12 max(1, cost), deg = rows + segments -- the duality gap at the
stop (mu <= tol, gap = deg mu), counted twice.

General polytopes (every n = 1..8; the boxes above leave A' diag(lam / s) A diagonal and run n = 1, 2, 3, 8 only), all with closed
forms but the bent chains, all held to that same bound and to nothing wider:
  moved       the corridor, the elbow and a staircase in a random orthogonal frame, translated, every row scaled by 10**U(-2, 2);
  line        a straight line between two points through random polytopes (n + 2 or 40 random facets and a box: up to 112 rows
              per point), at 9 points and at 31 .. 34, 63 .. 65 and 97 points (the chain is staged 32 blocks at a time);
  thin        the same with consecutive regions overlapping by a slab of width 1e-1, 1e-3, 1e-4;
  far         the same 1e2 and 1e4 from the origin;
  reflection  a path that has to touch a plane between its ends: an active facet, a segment of length zero;
  intervals   n = 1, where the problem is a linear program: chains of intervals against HiGHS;
  bent        random walks through regions of three different row counts, against the host solver;
  single      a path of one region;
  wide_call   300 pieces of one chain of 40 regions in one call.
The exact value of a case with point ends is the distance between the end BOXES (half-width 1e-6, axis-aligned before the move), so
that nothing of the order 1e-6 has to be allowed.  Deliberately outside: centres 1e6 from the origin (the host solver fails there
at n = 2), overlaps thinner than 1e-4 (the emulation needs about 80 of its 100 iterations at 1e-5)."""
import ctypes as C
import os

import numpy as np

from gcs_admm_amd.graph import chebyshev_center, convert_pt_to_polytope
from hostemu_lib import emu_library
from gcs_admm_amd.rounding import solve_path_restriction

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gcs_admm_amd", "csrc")
SRC = os.path.join(HERE, "hostemu", "restrict_emu.cpp")
TOL, MAX_ITER = 1e-10, 100
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2
RECORDS = {"benchmark1": 3.236065, "benchmark2": 7.413745, "benchmark3": 60.177021, "benchmark4": 32.627198}


# ---- cases: (label, n, polys, path, exact cost or None) ----
def box(centre, half=0.6):
    c = np.asarray(centre, float)
    n = len(c)
    return np.vstack([np.eye(n), -np.eye(n)]), np.hstack([c + half, -(c - half)])


def _embed(c2, n):
    c = np.zeros(n); c[:min(n, 2)] = c2[:min(n, 2)]
    return c


def corridor(k, n):
    return f"corridor-k{k}-n{n}", n, [box(_embed([i, 0.0], n)) for i in range(k)], list(range(k)), (k - 1) - 1.2


def staircase(K):
    cen = [(0.0, 0.0)]
    for i in range(K):
        cen += [(i + 1.0, float(i)), (i + 1.0, i + 1.0)]
    return f"staircase-K{K}", 2, [box(c) for c in cen], list(range(2 * K + 1)), np.sqrt(2.0) * (K - 1.2)


ELBOW = [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (2.0, 1.0), (2.0, 2.0)]


def elbow(n=2):
    return f"elbow-n{n}", n, [box(_embed(c, n)) for c in ELBOW], list(range(5)), 1.6


def all_zero():
    return "all-zero", 2, [box(c) for c in [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)]], [0, 1, 2], 0.0


def exact_cases():
    out = [corridor(3, n) for n in (1, 2, 3, 8)] + [corridor(70, 2), corridor(130, 2)]
    return out + [staircase(K) for K in (3, 10, 35)] + [elbow(), all_zero()]


def with_point_terminals(case, analytic):
    """the case with 's' / 't' as points (convert_pt_to_polytope) at the centres of its first and last box; the analytic value holds
    up to 2 sqrt(n) 1e-6: the end points may move inside their boxes"""
    label, n, polys, path, _ = case
    s = 0.5 * (polys[0][1][:n] - polys[0][1][n:]); t = 0.5 * (polys[-1][1][:n] - polys[-1][1][n:])
    P = len(polys)
    return label + "-points", n, polys + [convert_pt_to_polytope(s), convert_pt_to_polytope(t)], [P] + path + [P + 1], analytic


def point_cases():
    """the corridor (straight line between the centres: k - 1) at n = 1, 2, 3, 8 and the elbow, which lives in a plane, at n = 2, 3, 8
    (round the corner (1.4, 0.6) of the third box: 2 sqrt(1.4^2 + 0.6^2))"""
    return [with_point_terminals(corridor(4, n), 3.0) for n in (1, 2, 3, 8)] + \
           [with_point_terminals(elbow(n), 2.0 * np.hypot(1.4, 0.6)) for n in (2, 3, 8)]


def mixed_rows_case():
    """n = 3: regions of 6 and 7 rows mixed (a box, or a box plus a redundant cut), on a bent chain"""
    cen = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1)]
    polys = []
    for i, c in enumerate(cen):
        A, b = box(np.array(c, float))
        if i % 2:
            a = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
            A = np.vstack([A, a]); b = np.hstack([b, a @ np.array(c, float) + 2.0])       # outside the box's corners (0.6 sqrt 3 = 1.04)
        polys.append((A, b))
    return "mixed-rows-n3", 3, polys, list(range(len(cen))), None


# ---- general polytopes: (label, n, polys, path, exact cost or None), seeded, the same on the CPU and on the GPU ----
def rand_orth(n, rng):
    """a random orthogonal matrix: QR of a Gaussian matrix, the signs of R's diagonal fixed"""
    Qm, Rm = np.linalg.qr(rng.standard_normal((n, n)))
    return Qm * np.sign(np.diag(Rm))


def move(polys, Q, t, rng, scale=True):
    """every region under x -> Q x + t: (A, b) becomes (A Q', b + A Q' t); then every row times its own 10**U(-2, 2) (``scale``).
    Lengths, and with them every exact cost, stay as they are."""
    out = []
    for A, b in polys:
        A2 = np.asarray(A, float) @ Q.T
        b2 = np.asarray(b, float) + A2 @ t
        if scale:
            f = 10.0 ** rng.uniform(-2.0, 2.0, len(b2))
            A2 = A2 * f[:, None]; b2 = b2 * f
        out.append((A2, b2))
    return out


def rand_poly(c, n, m, rng, rin, rout, R):
    """``m`` random unit normals at distances U(rin, rout) from ``c``, and the box c +- R: bounded, contains the ball of radius
    ``rin`` about ``c``; m + 2n rows"""
    c = np.asarray(c, float)
    a = rng.standard_normal((m, n))
    a /= np.linalg.norm(a, axis=1)[:, None]
    return np.vstack([a, np.eye(n), -np.eye(n)]), np.hstack([a @ c + rng.uniform(rin, rout, m), c + R, -(c - R)])


def unit(n, rng):
    d = rng.standard_normal(n)
    return d / np.linalg.norm(d)


def box_distance(s, t, eps=1e-6):
    """distance between the boxes of half-width ``eps`` about s and t (convert_pt_to_polytope)"""
    return float(np.linalg.norm(np.maximum(0.0, np.abs(np.asarray(t, float) - np.asarray(s, float)) - 2.0 * eps)))


def moved_case(case, seed):
    """family 1: an exact case of boxes in a random frame, at a random place, with row norms between 1e-2 and 1e2"""
    label, n, polys, path, exact = case
    rng = np.random.default_rng(seed)
    return label + "-moved", n, move(polys, rand_orth(n, rng), rng.uniform(-3.0, 3.0, n), rng), path, exact


def moved_cases():
    return [moved_case(corridor(5, n), 100 + n) for n in range(2, 9)] + [moved_case(elbow(n), 120 + n) for n in range(2, 9)] + \
           [moved_case(staircase(3), 140)]


def line_case(n, k, m, seed, w=None, shift=None, tag="line"):
    """family 2: the straight line from s = 0 to t = (k - 1) d through k random polytopes about s + i d, each holding the ball of
    radius 0.6 about its centre; the ends are points.  The scene lists the two points first, then the regions; the path has k + 3
    points.  ``w`` (family 3): every region also lies in the slab of width 1 + w about its centre across d, so that consecutive
    regions overlap by a slab of width w.  ``shift`` (family 4): no row scaling, the translation is ``shift`` along (1, .., 1) /
    sqrt n.  Exact: the distance between the end boxes, which are axis-aligned before the move."""
    rng = np.random.default_rng(seed)
    d = unit(n, rng)
    s, t = np.zeros(n), (k - 1) * d
    regions = []
    for i in range(k):
        c = s + i * d
        A, b = rand_poly(c, n, m, rng, 0.6, 1.2, 3.0)
        if w is not None:
            A = np.vstack([A, d, -d]); b = np.hstack([b, d @ c + 0.5 * (1.0 + w), -(d @ c) + 0.5 * (1.0 + w)])
        regions.append((A, b))
    polys = [convert_pt_to_polytope(s), convert_pt_to_polytope(t)] + regions
    Q = rand_orth(n, rng)
    if shift is None:
        polys = move(polys, Q, rng.uniform(-3.0, 3.0, n), rng)
    else:
        polys = move(polys, Q, shift * np.ones(n) / np.sqrt(n), rng, scale=False)
    label = f"{tag}-n{n}-k{k}-m{m}" + (f"-w{w:g}" if w is not None else "") + (f"-at{shift:g}" if shift is not None else "")
    return label, n, polys, [0] + list(range(2, k + 2)) + [1], box_distance(s, t)


CHUNK_POINTS = (31, 32, 33, 34, 63, 64, 65, 97)       # around one and two full chunks of the chain (CHUNK = 32), and a fourth chunk


def line_cases():
    """n = 1..8 with few rows and with more rows per point (84 .. 112) than the workgroup has lanes; n = 5 and 8 at the chunk edges"""
    return [line_case(n, 6, n + 2, 200 + n) for n in range(1, 9)] + [line_case(n, 6, 40, 220 + n) for n in range(1, 9)] + \
           [line_case(n, pts - 3, n + 2, 240 + 10 * n + i) for n in (5, 8) for i, pts in enumerate(CHUNK_POINTS)]


THIN = (1e-1, 1e-3, 1e-4)     # 1e-4: the emulation needs at most 0.8 MAX_ITER Newton iterations there (test_thin_overlaps_leave_headroom)


def thin_cases():
    """family 3: consecutive regions overlap by a slab of width w"""
    return [line_case(n, 6, n + 2, 400 + 10 * n + i, w=w, tag="thin") for n in (2, 3, 6) for i, w in enumerate(THIN)]


def far_cases():
    """family 4: 1e2 and 1e4 from the origin, unit row norms.  At 1e6 the host solver (conic.py) itself fails at n = 2: outside the
    contract, not tested."""
    return [line_case(n, 6, n + 2, 500 + 10 * n + i, shift=sh, tag="far") for n in (2, 6) for i, sh in enumerate((1e2, 1e4))]


def reflection_case(n, seed):
    """family 5: from s = (-1.3, 0.8, 0..) to t = (0.9, 0.5, 0..) through x_2 >= 0, x_2 <= 0.05, x_2 >= 0 (within |x| <= 3): the
    shortest path touches the plane x_2 = 0.05 in one point, so a segment vanishes and one facet is active with a multiplier away
    from any symmetry.  Exact: the distance from the box of s to the mirror image of the box of t."""
    rng = np.random.default_rng(seed)
    s = np.zeros(n); s[:2] = (-1.3, 0.8)
    t = np.zeros(n); t[:2] = (0.9, 0.5)
    lo_up = np.full(n, -3.0); lo_up[1] = 0.0
    hi_dn = np.full(n, 3.0); hi_dn[1] = 0.05
    eye = np.vstack([np.eye(n), -np.eye(n)])
    up = (eye, np.hstack([np.full(n, 3.0), -lo_up]))
    down = (eye, np.hstack([hi_dn, np.full(n, 3.0)]))
    polys = move([convert_pt_to_polytope(s), convert_pt_to_polytope(t), up, down], rand_orth(n, rng), rng.uniform(-3.0, 3.0, n), rng)
    mirror = t.copy(); mirror[1] = 2.0 * 0.05 - t[1]
    return f"reflection-n{n}", n, polys, [0, 2, 3, 2, 1], box_distance(s, mirror)


def reflection_cases():
    return [reflection_case(n, 600 + n) for n in range(2, 9)]


def interval_case(seed):
    """family 6, n = 1: a chain of 8 to 12 overlapping intervals on a random walk, rows of unequal scale.  The problem is a linear
    program, min sum t_j with +-(q_{j+1} - q_j) <= t_j; exact is the optimum HiGHS finds for it."""
    from scipy.optimize import linprog
    rng = np.random.default_rng(seed)
    k = int(rng.integers(8, 13))
    half = rng.uniform(0.5, 1.5, k)
    cen = np.zeros(k)
    for i in range(1, k):
        cen[i] = cen[i - 1] + rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 0.9) * (half[i - 1] + half[i])
    lo, hi = cen - half, cen + half
    polys = []
    for i in range(k):
        f = 10.0 ** rng.uniform(-2.0, 2.0, 2)
        polys.append((np.array([[f[0]], [-f[1]]]), np.array([f[0] * hi[i], -f[1] * lo[i]])))
    path = list(range(k))
    qlo = [lo[0]] + [max(lo[j - 1], lo[j]) for j in range(1, k)] + [lo[-1]]
    qhi = [hi[0]] + [min(hi[j - 1], hi[j]) for j in range(1, k)] + [hi[-1]]
    c = np.hstack([np.zeros(k + 1), np.ones(k)])
    rows = []
    for j in range(k):
        for sg in (1.0, -1.0):
            r = np.zeros(2 * k + 1); r[j + 1] = sg; r[j] = -sg; r[k + 1 + j] = -1.0
            rows.append(r)
    res = linprog(c, A_ub=np.array(rows), b_ub=np.zeros(2 * k), bounds=list(zip(qlo, qhi)) + [(0.0, None)] * k, method="highs")
    assert res.status == 0, res.message
    return f"intervals-{seed}-k{k}", 1, polys, path, float(res.fun)


def interval_cases():
    return [interval_case(700 + i) for i in range(10)]


def bent_case(n, seed, k=7):
    """family 7: centres on a random walk of unit steps, regions of n + 3, n + 8 and n + 13 random facets (plus the box c +- 1) in
    turn, the ends are points at the first and the last centre.  No closed form: the host solver is the yardstick."""
    rng = np.random.default_rng(seed)
    cen, d = [np.zeros(n)], unit(n, rng)
    for _ in range(k - 1):
        d = d + 0.8 * rng.standard_normal(n) / np.sqrt(n)
        d /= np.linalg.norm(d)
        cen.append(cen[-1] + d)
    regions = [rand_poly(c, n, n + 3 + 5 * (i % 3), rng, 0.6, 0.75, 1.0) for i, c in enumerate(cen)]
    polys = [convert_pt_to_polytope(cen[0]), convert_pt_to_polytope(cen[-1])] + regions
    return f"bent-n{n}", n, polys, [0] + list(range(2, k + 2)) + [1], None


def bent_cases():
    return [bent_case(n, 800 + n) for n in range(2, 9)]


def single_cases():
    """family 8: one region, as a path of one step and of two: both points may coincide, the cost is 0"""
    out = []
    for n in (1, 4, 7):
        rng = np.random.default_rng(900 + n)
        polys = move([rand_poly(rng.uniform(-1.0, 1.0, n), n, n + 2, rng, 0.6, 1.2, 3.0)], rand_orth(n, rng), rng.uniform(-3.0, 3.0, n), rng)
        out += [(f"single-n{n}", n, polys, [0], 0.0), (f"single-twice-n{n}", n, polys, [0, 0], 0.0)]
    return out


FAMILIES = {"moved": moved_cases, "line": line_cases, "thin": thin_cases, "far": far_cases, "reflection": reflection_cases,
            "intervals": interval_cases, "bent": bent_cases, "single": single_cases}
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def closed_form_cases():
    """every new case with an exact cost"""
    return [c for name in FAMILIES if name != "bent" for c in family(name)]


def general_cases():
    return closed_form_cases() + family("bent")


WIDE_N, WIDE_CHAIN, WIDE_EXTRA, WIDE_PATHS, WIDE_W = 5, 40, 20, 300, 0.1
WIDE_SOLO = (0, 1, 2, 57, 123, 211, 298, 299)       # solved again alone; 0 is the shortest path and 299 the longest


def wide_call():
    """family 9, n = 5: one scene of a chain of 40 regions along a line and 20 further regions, and 300 paths in one call, each a
    contiguous piece of the chain of 1 to 40 regions.  The chain is that of family 3 with w = 0.1: the ends of a piece are regions,
    not points, and only the slabs pin where it has to enter and leave -- a piece of L >= 3 regions costs (L - 2) - w, a shorter one
    0.  Returns (n, polys, paths, starts, exact costs)."""
    rng = np.random.default_rng(1000)
    n, K, w = WIDE_N, WIDE_CHAIN, WIDE_W
    d = unit(n, rng)
    polys = []
    for i in range(K):
        c = i * d
        A, b = rand_poly(c, n, n + 2, rng, 0.6, 1.2, 3.0)
        polys.append((np.vstack([A, d, -d]), np.hstack([b, d @ c + 0.5 * (1.0 + w), -(d @ c) + 0.5 * (1.0 + w)])))
    polys += [rand_poly(rng.uniform(-5.0, 5.0, n), n, n + 2 + 3 * (i % 4), rng, 0.6, 1.2, 3.0) for i in range(WIDE_EXTRA)]
    polys = move(polys, rand_orth(n, rng), rng.uniform(-3.0, 3.0, n), rng)
    pieces = [(0, 1), (K - 1, 1), (3, 2)]
    while len(pieces) < WIDE_PATHS - 1:
        L = int(rng.integers(1, K + 1))
        pieces.append((int(rng.integers(0, K - L + 1)), L))
    pieces.append((0, K))
    paths = [list(range(a, a + L)) for a, L in pieces]
    centre = {}

    def cen(*regs):
        if regs not in centre:
            centre[regs] = chebyshev_center(np.vstack([polys[r][0] for r in regs]), np.hstack([polys[r][1] for r in regs]))
        return centre[regs]
    starts = [np.array([cen(p[0])] + [cen(p[j - 1], p[j]) for j in range(1, len(p))] + [cen(p[-1])]) for p in paths]
    return n, polys, paths, starts, [max(0.0, (L - 2) - w) if L >= 3 else 0.0 for _, L in pieces]


def benchmark_case(name, y_e=None):
    """the most probable path of a benchmark under the activations ``y_e`` (the oracle's run)"""
    from gcs_admm_amd.cases import fixture_sets
    from gcs_admm_amd.rounding import most_probable_path
    As, bs, n, _, _ = fixture_sets(name)
    keys = list(As)
    E = list(y_e)
    I_out = {v: [e for e in E if e[0] == v] for v in keys}
    path = most_probable_path(y_e, I_out)
    return name, n, [(np.asarray(As[v], float), np.asarray(bs[v], float)) for v in keys], [keys.index(v) for v in path], None


def oracle_activations(oracle_lib, name):
    """relaxed edge activations of a benchmark from the CPU oracle's run, as tests/test_rounding.py takes them"""
    from gcs_admm_amd import IPM_TOL
    from gcs_admm_amd.cases import load_fixture
    _, g = load_fixture(name)
    o = oracle_lib.Oracle(g, ipm_tol=IPM_TOL)
    o.run(nthreads=4)
    E = g.edges_as_keys()
    return g.keys, E, {e: float(o.zedge[2 * g.n, i]) for i, e in enumerate(E)}


# ---- what the checks need ----
def point_rows(polys, path):
    """(A, b) of every point of the path: the rows of r_{j-1}, then those of r_j"""
    k = len(path)
    regs = [[path[0]]] + [[path[j - 1], path[j]] for j in range(1, k)] + [[path[-1]]]
    return [(np.vstack([polys[r][0] for r in reg]), np.hstack([polys[r][1] for r in reg])) for reg in regs]


def degree(polys, path):
    return sum(len(b) for _, b in point_rows(polys, path)) + len(path)


def bound(polys, path, cost, tol=TOL):
    return 2.0 * degree(polys, path) * tol + 1e-12 * max(1.0, abs(cost))


def host_start(polys, path):
    """Chebyshev centres of the one- or two-region intersections: the start of solve_path_restriction"""
    return np.array([chebyshev_center(A, b) for A, b in point_rows(polys, path)])


_starts = {}


def case_start(case):
    """``host_start`` of a case, computed once per label (the labels are unique)"""
    if case[0] not in _starts:
        _starts[case[0]] = host_start(case[2], case[3])
    return _starts[case[0]]


def host_cost(polys, path, n):
    cost, xs = solve_path_restriction({i: A for i, (A, _) in enumerate(polys)}, {i: b for i, (_, b) in enumerate(polys)}, n, path)
    assert xs is not None
    return cost


def assert_points_feasible(polys, path, pts):
    for (A, b), x in zip(point_rows(polys, path), pts):
        assert np.all(A @ x - b <= 1e-9 * np.maximum(1.0, np.abs(b))), (A @ x - b).max()


def assert_solution(case, pts, cost, its, st, reference=None, extra=0.0, max_iter=MAX_ITER):
    """the gates of one case: status, iteration limit, rows, and the cost against the exact answer (or ``reference``: the host's cost,
    which brings a bound of its own; ``extra``: what the analytic value of a point-terminal case is allowed on top)"""
    label, n, polys, path, exact = case
    print(f"{label}: cost {cost!r} exact {exact!r} host {reference!r} iterations {its} status {st} bound {bound(polys, path, cost):.3e}")
    assert st == 0, (label, st)
    assert 0 <= its <= max_iter, (label, its)
    assert np.isclose(cost, sum(np.linalg.norm(pts[j + 1] - pts[j]) for j in range(len(path))), rtol=1e-13, atol=1e-15), label
    assert_points_feasible(polys, path, pts)
    if exact is not None:
        assert abs(cost - exact) <= bound(polys, path, cost) + extra, (label, cost - exact)
    if reference is not None:
        assert abs(cost - reference) <= 2.0 * bound(polys, path, cost), (label, cost - reference)


# ---- CSR form of a call ----
def flatten(n, polys, paths, starts):
    """(poly_ptr, A, b, path_ptr, path_poly, start): the arrays of gcsadmm_scene_restrict_paths; path p's points at (path_ptr[p] + p) n"""
    ptr = np.zeros(len(polys) + 1, np.int32); ptr[1:] = np.cumsum([len(b) for _, b in polys])
    A = np.ascontiguousarray(np.vstack([np.asarray(a, float).reshape(-1, n) for a, _ in polys]))
    b = np.ascontiguousarray(np.hstack([np.asarray(v, float).ravel() for _, v in polys]))
    pp = np.zeros(len(paths) + 1, np.int32); pp[1:] = np.cumsum([len(p) for p in paths])
    poly = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32) for p in paths]) if paths else np.zeros(0, np.int32), np.int32)
    start = np.ascontiguousarray(np.concatenate([np.asarray(s, float).reshape(-1, n) for s in starts]) if starts else np.zeros((0, n)))
    assert start.shape[0] == int(pp[-1]) + len(paths)
    return ptr, A, b, pp, poly, start


def split_points(n, pp, flat):
    return [flat[int(pp[p]) + p:int(pp[p + 1]) + p + 1] for p in range(len(pp) - 1)]


# ---- the host emulation ----
_lib = None


def emu():
    global _lib
    if _lib is None:
        _lib = emu_library("restrictemu")
        _lib.restrict_emu_error.restype = C.c_char_p
        _lib.restrict_emu_ws_doubles.restype = C.c_longlong
        _lib.restrict_emu_ws_doubles.argtypes = [C.c_int, C.c_longlong, C.c_longlong]
        _lib.restrict_emu_solve.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 4
        _lib.restrict_emu_plan.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    return _lib


def emu_raw(n, ptr, A, b, pp, poly, start, tol=TOL, max_iter=MAX_ITER, reverse=False):
    """restrict_emu_solve on the arrays: (return code, points, cost, iterations, status)"""
    num = len(pp) - 1
    pts = np.full_like(start, np.nan); cost = np.full(num, np.nan); its = np.full(num, -7, np.int32); st = np.full(num, -7, np.int32)
    rc = emu().restrict_emu_solve(n, len(ptr) - 1, ptr.ctypes.data, A.ctypes.data, b.ctypes.data, num, pp.ctypes.data, poly.ctypes.data,
                                  start.ctypes.data, tol, max_iter, int(reverse), pts.ctypes.data, cost.ctypes.data, its.ctypes.data, st.ctypes.data)
    return rc, pts, cost, its, st


def emu_solver(reverse=False):
    def solve(n, polys, paths, starts, tol=TOL, max_iter=MAX_ITER):
        arrays = flatten(n, polys, paths, starts)
        rc, pts, cost, its, st = emu_raw(n, *arrays, tol=tol, max_iter=max_iter, reverse=reverse)
        assert rc == OK, emu().restrict_emu_error().decode()
        return split_points(n, arrays[3], pts), cost, its, st
    return solve


def device_solver(device=0):
    """gcsadmm_scene_restrict_paths through DeviceScene.restrict_paths, one scene per call"""
    from gcs_admm_amd.scene import DeviceScene

    def solve(n, polys, paths, starts, tol=TOL, max_iter=MAX_ITER):
        with DeviceScene(polys, device) as sc:
            return sc.restrict_paths(paths, starts, tol=tol, max_iter=max_iter)
    return solve
