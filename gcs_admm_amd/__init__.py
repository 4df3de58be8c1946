"""MI355X-native ADMM loop for shortest paths in graphs of convex sets
(drop-in for the hot path of the reference's admm_solver_v3.py)."""
from .graph import (GcsGraph, build_graph, convert_pt_to_polytope, delta, graph_from_sets,  # noqa: F401
                    lattice_boxes, polytopes_overlap)
from .cases import load_fixture  # noqa: F401
from .batch import BatchSolver  # noqa: F401  (many small problems in one set of launches; needs the GPU only when one is made)
from .queries import SceneQueries  # noqa: F401  (many start / goal queries on one resident scene)
from .transfer import StateSnapshot  # noqa: F401  (replanning: a solved state kept to seed the next query)

# Barrier parameter at which a vertex solve stops (gcsadmm_params.ipm_tol).  MOSEK's default relative gap behind the reference's
# SolveInParallel (admm_solver_v3.py:490) is ~1e-8.  Swept on the oracle in round 4 (profiles/r04/README.md): 1e-9, 3e-9 and 5e-9 keep
# every gate -- stop iterations 39 / 100 / 508 / 465 of the reference's records and 959 on the 10k lattice exact, every entry of the
# reference's residual traces inside 2e-4 + 1e-3 |g|, the eps = 1e-6 run of benchmark4 converging to the monolithic optimum -- while
# 1e-8 loses two of them (the 10k lattice stops at 958, the eps = 1e-6 run no longer converges).  3e-9: 8 % fewer Newton iterations.
IPM_TOL = 3e-9

__all__ = ["GcsGraph", "build_graph", "convert_pt_to_polytope", "delta", "graph_from_sets", "lattice_boxes",
           "polytopes_overlap", "load_fixture", "BatchSolver", "SceneQueries", "StateSnapshot", "IPM_TOL"]
