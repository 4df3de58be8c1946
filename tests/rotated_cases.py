"""Vertex-step cases on ROTATED polytopes in R^3 .. R^8 (test_rotated_steps.py: the host builds; test_gpu_rotated_steps.py: the device).

Outside n = 2 every other vertex solve of the suite is on a canonical box [I; -I]: every off-diagonal product A[j,k] A[j,l] in K_h, X_e
and the facet sums is then an exact zero, so the dense-row path of the generic workgroup program (csrc/vertex_wg.h, BOX = false) gets
no test of those terms.  A case here is a lattice_boxes(4, 3, n, seed) graph -- 14 vertices, 12 of them generic, degree up to 6 -- whose
every polytope is rotated by ONE orthogonal Q: A' = A Q', b unchanged, interior' = interior Q'.  The sub-problems are mathematically the
same (the objective is a sum of norms and squared distances), so the axis-aligned lattice solved by the oracle is a reference for the
rotated solve that does not share the dense-row code ("equivariance": rotate the two point blocks of every column, leave y alone).

These are VERTEX-STEP cases with GIVEN edges, not scenes: the edge list is the lattice's own, and the graph is assembled by
_finish_graph directly.  graph_from_sets would centre the unknowns at its Chebyshev LP's centre, which is not the rotated centre of a
non-cubic box, and equivariance then holds only to ~5e-6 (measured).  s and t stay point terminals, at Q p.

cuts > 0: every cell gains `cuts` further rows (a Q', a . cen + U(0.25, 0.45)) with |a| = 1 -- the axis-aligned side the rows
(a, same right-hand side) -- so the row counts differ vertex by vertex: 2n for the terminals, 2n + cuts for the cells.

A case is named by (n, lattice seed, rotation seed, cuts).  The rotation of seed r is the Q of np.linalg.qr(default_rng(r).normal(size =
(n, n))); the census pairs lattice seed 1 + k with rotation seed 100 k + n, k = 0 .. 7.
"""
import numpy as np

from gcs_admm_amd.graph import _finish_graph, lattice_boxes

NX_CELLS, NY_CELLS = 4, 3
STEPS = 12


def rotation(n, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(n, n)))
    return q


def rotated_pair(n, lattice_seed, rotation_seed, cuts=0):
    """(axis-aligned graph, rotated graph, Q): the lattice (with its cut rows, unrotated) and the same polytopes rotated by Q; both have
    the lattice's edges, so their incidence structure is identical"""
    g = lattice_boxes(NX_CELLS, NY_CELLS, n=n, seed=lattice_seed)
    Q = rotation(n, rotation_seed)
    rng = np.random.default_rng([rotation_seed, cuts])
    base, rot = [], []
    for v in range(g.num_vertices):
        A = g.poly_A[g.poly_ptr[v]:g.poly_ptr[v + 1]]
        b = g.poly_b[g.poly_ptr[v]:g.poly_ptr[v + 1]]
        if v in (g.src, g.dst):              # a point terminal stays one: the same small canonical box about Q p
            p = 0.5 * (b[:n] - b[n:])
            base.append((A, b))
            rot.append((A, b + np.hstack([Q @ p - p, -(Q @ p - p)])))
            continue
        if cuts:
            a = rng.normal(size=(cuts, n))
            a /= np.linalg.norm(a, axis=1)[:, None]
            A = np.vstack([A, a])
            b = np.hstack([b, a @ g.interior[v] + rng.uniform(0.25, 0.45, size=cuts)])
        base.append((A, b))
        rot.append((A @ Q.T, b))
    interior = np.asarray(g.interior)
    interior_rot = interior @ Q.T
    for v in (g.src, g.dst):                 # (bit for bit the centre of the terminal's box)
        b = rot[v][1]
        interior_rot[v] = 0.5 * (b[:n] - b[n:])
    fin = lambda polys, cen: _finish_graph(n, list(g.keys), g.edge_tail, g.edge_head, polys, cen, g.src, g.dst)
    return fin(base, interior), fin(rot, interior_rot), Q


def rotated_graph(n, lattice_seed, rotation_seed, cuts=0):
    return rotated_pair(n, lattice_seed, rotation_seed, cuts)[1]


def rotate_state(a, Q):
    """a [2n + 1, columns] state array of the axis-aligned side in the rotated frame: both point blocks rotated, y as it is"""
    n = Q.shape[0]
    out = np.array(a, dtype=np.float64, copy=True)
    out[0:n] = Q @ a[0:n]
    out[n:2 * n] = Q @ a[n:2 * n]
    return out


def census_seeds(n):
    """[(lattice seed, rotation seed)] of the failure census at dimension n"""
    return [(1 + k, 100 * k + n) for k in range(8)]


# (n, lattice seed, rotation seed, cuts).  cuts 0 at n = 3 .. 8; cuts 2, 3, 4, 5 at n = 3, 4, 6, 8.  The seeds at n = 5 .. 8 are ones
# whose vertex 13 (the cell that holds t, y_v -> 1) ended in a non-finite Newton step before the rule of gcs_math::step_finite (the
# census of test_rotated_steps.py quotes them); (6, 2, 106, 0) cold is the first one found: step 5 failed at iteration 11
CASES = [
    (3, 1, 3, 0), (4, 1, 4, 0), (5, 7, 605, 0), (6, 2, 106, 0), (7, 3, 207, 0), (8, 4, 308, 0),
    (3, 1, 3, 2), (4, 1, 4, 3), (6, 2, 106, 4), (8, 4, 308, 5),
]
REPRO = (6, 2, 106, 0)


def case_id(case):
    return "n{}-lat{}-rot{}-cuts{}".format(*case)
