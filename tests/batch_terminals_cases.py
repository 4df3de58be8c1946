"""The graphs with terminals that are regions that the batch-terminal tests share (test_batch_terminals_plan.py on the host,
test_gpu_batch_terminals.py on the GPU), restated here from the modules that first made them (scaled_cases.region_row / region_scene,
test_gpu_configs._region_star) so that both files name one member the same way, with what each member's create plan must say about
its terminals: (terminals, threads, work arrays in LDS)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _box_rows(n):
    return np.vstack([np.eye(n), -np.eye(n)])


def region_row():
    """three boxes in a row, the outer two are the terminals: s = [0,1] x [0,1], t = [2,3] x [0,1], between them [0.8,2.2] x [0,1]"""
    from gcs_admm_amd.graph import graph_from_sets
    A = _box_rows(2)
    box = lambda x0, x1, y0, y1: (A, np.array([x1, y1, -x0, -y0], float))
    As, bs = {}, {}
    As['s'], bs['s'] = box(0, 1, 0, 1); As['t'], bs['t'] = box(2, 3, 0, 1); As[0], bs[0] = box(0.8, 2.2, 0, 1)
    return graph_from_sets(As, bs, 2)


def region_scene(seed, half=0.35):
    """a 4 x 4 polygon scene (tools/scale_demo.py) whose terminals are boxes of half-width ``half`` about the points they were"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from scale_demo import polygon_scene
    from gcs_admm_amd.graph import graph_from_sets
    As, bs = polygon_scene(4, seed=seed, m=3 + seed % 4)
    A = _box_rows(2)
    for key in ('s', 't'):
        pt = 0.5 * (bs[key][:2] - bs[key][2:])
        As[key], bs[key] = A, np.hstack([pt + half, -pt + half])
    return graph_from_sets(As, bs, 2)


def region_star(n, spokes, seed=0, source=None):
    """a source that is the box [-1, 1]^n (or the polytope ``source`` = (A, b)) overlapping ``spokes`` small boxes on a ring,
    neighbours on the ring joined; the target a point in the last of them (edges given).  The source's sub-problem has ``spokes``
    live blocks."""
    from gcs_admm_amd.graph import convert_pt_to_polytope, graph_from_sets
    rng = np.random.default_rng(seed)
    A = _box_rows(n)
    As, bs = {}, {}
    As['s'], bs['s'] = source if source is not None else (A, np.hstack([np.full(n, 1.0), np.full(n, 1.0)]))
    edges = []
    for k in range(spokes):
        c = np.zeros(n); ang = 2 * np.pi * k / spokes
        c[0], c[1] = 1.1 * np.cos(ang), 1.1 * np.sin(ang)
        c[2:] = rng.uniform(-0.3, 0.3, n - 2)
        h = rng.uniform(0.3, 0.4, n)
        As[k], bs[k] = A, np.hstack([c + h, -c + h])
        edges += [('s', k), (k, 's')]
    last = spokes - 1
    ctr = 0.5 * (bs[last][:n] - bs[last][n:])
    As['t'], bs['t'] = convert_pt_to_polytope(ctr + 0.1)
    edges += [(last, 't'), ('t', last)]
    for k in range(spokes):
        edges += [(k, (k + 1) % spokes), ((k + 1) % spokes, k)]
    keys = ['s', 't'] + list(range(spokes))
    return graph_from_sets({k: As[k] for k in keys}, {k: bs[k] for k in keys}, n, edges=edges)


# name -> (graph, (n_term, term_threads, term_lds_doubles > 0) of its create plan with vertex_program = 3)
# The groups a batch can have are {64, 256} threads x {LDS, workspace}.  One wavefront is chosen while no phase has more than 256 rows
# (live edges x 2 x facets) and LDS while the largest work array fits 48 KB.  The cases below reach (64, LDS) and (256, workspace);
# EXTRA has one small graph for each of the remaining two.
CASES = {
    "row": (region_row, (2, 64, True)),
    "scene1": (lambda: region_scene(1), (2, 64, True)),
    "scene2": (lambda: region_scene(2, half=0.2), (2, 64, True)),
    "star3": (lambda: region_star(3, 8, seed=3), (1, 64, True)),
    "star3b": (lambda: region_star(3, 8, seed=4), (1, 64, True)),
    "star6": (lambda: region_star(6, 30, seed=6), (1, 256, False)),
    "star8": (lambda: region_star(8, 6, seed=8), (1, 64, True)),
    "star8b": (lambda: region_star(8, 6, seed=9), (1, 64, True)),
}



def simplex_star(n=6, spokes=18, seed=1):
    """region_star with a SIMPLEX as the source: x_i >= -1, sum x_i <= sqrt(n) -- n + 1 facets instead of 2 n, so that 18 live edges
    are 252 rows (one wavefront) while the work arrays, 7 519 doubles, exceed 48 KB: the (64 threads, workspace) group"""
    return region_star(n, spokes, seed=seed, source=(np.vstack([-np.eye(n), np.ones((1, n))]), np.hstack([np.ones(n), [np.sqrt(n)]])))


# the two groups beyond those of the fixtures above, each reached by one small graph
EXTRA = {
    "star2x33": (lambda: region_star(2, 33, seed=2), (1, 256, True)),       # 33 live edges x 8 rows = 264 rows, 3 741 doubles
    "simplex6": (simplex_star, (1, 64, False)),
}

_graphs = {}


def graph(name):
    """the graph of CASES[name] or EXTRA[name], made once"""
    if name not in _graphs:
        _graphs[name] = {**CASES, **EXTRA}[name][0]()
    return _graphs[name]
