"""Replanning: the state of a solved problem, kept to seed the next one (gcsadmm_export_state / gcsadmm_import_state of
include/gcsadmm.h; csrc/state_transfer_core.h has the kernels' contract).

A planner on a resident scene asks almost the same query again every tick.  The relaxation is convex, so the loop converges from any
state, and from the state of the query before it needs a fraction of the iterations.  A ``StateSnapshot`` holds that state on the
device, named by stable vertex ids instead of by the numbering of one graph: ``BatchSolver.export_state`` writes one per member,
``BatchSolver.solve(seed=...)`` reads them into the members of another batch, whatever their graphs are, and
``SceneQueries.solve(keep=True)`` / ``solve(seed=...)`` do both with the scene's own ids.
"""
from __future__ import annotations

from . import abi


def check_vertex_ids(ids, num_vertices):
    """int32 [V] contiguous, every id >= 0, strictly ascending: what the library takes (it checks again)"""
    import numpy as np
    ids = np.ascontiguousarray(ids, np.int64).ravel()
    if len(ids) != num_vertices:
        raise ValueError(f"{num_vertices} vertex ids expected, {len(ids)} given")
    if len(ids) and (ids[0] < 0 or ids[-1] > 2 ** 31 - 1 or np.any(np.diff(ids) <= 0)):
        raise ValueError("vertex ids must lie in 0 .. 2^31 - 1 and ascend strictly with the vertex index")
    return ids.astype(np.int32)


class StateSnapshot:
    """Device tensors of one snapshot with room for ``V`` vertices and ``E`` edges of dimension ``n`` and state type ``state_dtype``
    ("f64" | "f32"): ``edge_key`` int64 [E], ``edge_words`` [5, c, E] (zedge, copy at tail and head, mu at tail and head),
    ``vertex_id`` int32 [V], ``vertex_words`` f64 [4n + 1, V] (xv, zv, yv), ``rho`` f64 [1].  ``c`` is the gcsadmm_snapshot over them;
    after an export ``V`` and ``E`` are the sizes written.  ``close()`` releases the tensors."""

    def __init__(self, n: int, state_dtype: str, V: int, E: int, device):
        import torch
        self.n, self.state_dtype, self.device = int(n), state_dtype, device
        tdtype = {"f64": torch.float64, "f32": torch.float32}[state_dtype]
        c = 2 * self.n + 1
        # (at least one entry each: an empty tensor has a null data pointer, which the ABI rejects)
        self.edge_key = torch.empty(max(E, 1), dtype=torch.int64, device=device)
        self.edge_words = torch.empty(5 * c * max(E, 1), dtype=tdtype, device=device)
        self.vertex_id = torch.empty(max(V, 1), dtype=torch.int32, device=device)
        self.vertex_words = torch.empty((4 * self.n + 1) * max(V, 1), dtype=torch.float64, device=device)
        self.rho = torch.empty(1, dtype=torch.float64, device=device)
        self.c = abi.Snapshot(n=self.n, state_dtype={"f64": abi.F64, "f32": abi.F32}[state_dtype], V=int(V), E=int(E),
                              edge_key=self.edge_key.data_ptr(), edge_words=self.edge_words.data_ptr(), vertex_id=self.vertex_id.data_ptr(),
                              vertex_words=self.vertex_words.data_ptr(), rho=self.rho.data_ptr())

    @property
    def V(self) -> int:
        return self.c.V

    @property
    def E(self) -> int:
        return self.c.E

    def arrays(self):
        """host copies shaped by the sizes written: edge_key [E], edge_words [5, c, E], vertex_id [V], vertex_words [4n + 1, V], rho [1]"""
        V, E, c = self.V, self.E, 2 * self.n + 1
        return dict(edge_key=self.edge_key[:E].cpu().numpy(), edge_words=self.edge_words[:5 * c * E].cpu().numpy().reshape(5, c, E),
                    vertex_id=self.vertex_id[:V].cpu().numpy(), vertex_words=self.vertex_words[:(4 * self.n + 1) * V].cpu().numpy().reshape(4 * self.n + 1, V),
                    rho=self.rho.cpu().numpy())

    def close(self):
        self.edge_key = self.edge_words = self.vertex_id = self.vertex_words = self.rho = self.c = None
