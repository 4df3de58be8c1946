"""Graphs of the fused-tail tests (test_fused_tail_plan.py on the host, test_gpu_fused_tail.py on the GPU): the smallest shapes at which
the one-launch iteration can go wrong."""
import numpy as np

from gcs_admm_amd.graph import convert_pt_to_polytope, graph_from_sets, lattice_boxes

EDGE_BLOCK = 256      # edges one edge workgroup holds (csrc/step_args.h)


def path3():
    """s, one box, t: one generic vertex (degree 2, 4 facets) and one workgroup that holds only the two closed-form vertices"""
    A = np.vstack([np.eye(2), -np.eye(2)])
    As, bs = {}, {}
    As['s'], bs['s'] = convert_pt_to_polytope([0.5, 0.5]); As['t'], bs['t'] = convert_pt_to_polytope([2.5, 0.5])
    As[0], bs[0] = A, np.array([3.0, 1.0, 0.0, 0.0])
    return graph_from_sets(As, bs, 2)


def _lattices():
    """(edges, columns, rows) of the box lattices up to 13 x 19, by edge count"""
    return sorted((lattice_boxes(c, r).num_edges, c, r) for c in range(1, 14) for r in range(c, 20))


def largest_fused_lattice():
    """the largest lattice whose edges fit one edge workgroup: the last edge thread is in use"""
    E, c, r = [x for x in _lattices() if x[0] <= EDGE_BLOCK][-1]
    assert E == EDGE_BLOCK, E
    return lattice_boxes(c, r)


def smallest_unfused_lattice():
    """the smallest lattice with more edges than one edge workgroup holds"""
    E, c, r = [x for x in _lattices() if x[0] > EDGE_BLOCK][0]
    return lattice_boxes(c, r)
