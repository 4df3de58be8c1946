"""Replanning without a device: the front end of the state transfer on a stand-in scene (the region serials of ``SceneQueries`` across
``add_regions`` / ``remove_regions``, the vertex ids of its query graphs, the ``keep`` / ``seed`` plumbing of ``solve``, the refusal
when order and serials disagree), and the claim itself on the CPU oracle: on benchmark4's regions a query seeded from the solution of
the query before it stops in at most half the iterations of the same query from zero, at the same rounded cost.

Measured on the oracle for the table of replanning_cases.py (cold / seeded iterations): shift 0.05: 419 / 7; 0.2: 418 / 11; 0.2 with
3 regions removed: 357 / 16; 0.5: 419 / 19; 0.5 with 6 removed: 362 / 24; rounded costs equal to every printed digit."""
import numpy as np
import pytest

import replanning_cases as R
from test_scene_edit import _queries, _regions


# ------------------------------------------------------------------------------------------- region serials and vertex ids
@pytest.fixture()
def edited():
    As, bs, n = _regions("benchmark4")
    keys = list(As)
    return As, bs, n, keys, _queries(As, bs, n, keys[:-5])


def _a_graph(sq, keep=None):
    c = sq.centers
    regs = sq.regions_at(np.vstack([c[0], c[-1]]))
    mask = None if keep is None else np.asarray(keep, bool)
    if mask is not None:
        mask[regs[0]] = True; mask[regs[1]] = True
    return sq._host_graph(c[0], c[-1], regs[0], regs[1], 1e-6, mask), mask


def test_serials_survive_every_edit(edited):
    As, bs, n, keys, sq = edited
    P = len(keys) - 5
    assert sq.serials == list(range(P))
    g, _ = _a_graph(sq)
    ids = sq.vertex_ids(g)
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1] + [r + 2 for r in range(P)]
    sq.add_regions({k: As[k] for k in keys[-5:-2]}, {k: bs[k] for k in keys[-5:-2]})
    assert sq.serials == list(range(P + 3))
    sq.remove_regions([keys[1], keys[P]])
    left = [r for r in range(P + 3) if r not in (1, P)]
    assert sq.serials == left and sq.keys == [keys[r] for r in left]
    sq.add_regions({keys[1]: As[keys[1]], keys[-1]: As[keys[-1]]}, {keys[1]: bs[keys[1]], keys[-1]: bs[keys[-1]]})
    assert sq.serials == left + [P + 3, P + 4]                      # a region that comes back is a new region: no serial is reused
    g, _ = _a_graph(sq)
    assert sq.vertex_ids(g).tolist() == [0, 1] + [r + 2 for r in sq.serials]
    # a pruned graph carries the serials of the regions it kept
    keep = np.arange(len(sq.keys)) % 3 == 0
    g, mask = _a_graph(sq, keep)
    assert g.num_vertices == 2 + int(mask.sum()) < 2 + len(sq.keys)
    assert sq.vertex_ids(g).tolist() == [0, 1] + [r + 2 for r, m in zip(sq.serials, mask) if m]
    # ... and a graph from before an edit still has its ids, as long as its regions are in the scene
    sq.remove_regions([sq.keys[4]]) if not mask[4] else sq.remove_regions([sq.keys[5]])
    assert sq.vertex_ids(g).tolist() == [0, 1] + [sq.serials[sq.keys.index(k)] + 2 for k in g.keys[2:]]
    sq.close()


def test_order_against_serials_is_refused_not_sorted(edited):
    *_, sq = edited
    g, _ = _a_graph(sq)
    sq.serials[2], sq.serials[3] = sq.serials[3], sq.serials[2]
    with pytest.raises(RuntimeError, match="serial numbers disagree"):
        sq.vertex_ids(g)
    sq.serials[2], sq.serials[3] = sq.serials[3], sq.serials[2]
    gone = sq.keys[2]
    sq.remove_regions([gone])
    with pytest.raises(ValueError, match="not in the scene"):
        sq.vertex_ids(g)
    sq.close()


# ------------------------------------------------------------------------------------------- keep and seed through solve
class _Member:
    def close(self):
        pass


class _Batch:
    """``BatchSolver`` as ``SceneQueries.solve`` uses it, recording its calls"""
    log = []

    def __init__(self, graphs, state_dtype, device=None, large=False, region_terminals=False):
        self.members = [_Member() for _ in graphs]
        _Batch.log.append(("init", len(graphs)))

    def solve(self, params=None, **kw):
        _Batch.log.append(("solve", kw))
        return [dict(iterations=1) for _ in self.members]

    def export_state(self, ids):
        _Batch.log.append(("export", [np.asarray(i).tolist() for i in ids]))
        return [("snapshot", k) for k in range(len(self.members))]

    def close(self):
        _Batch.log.append(("close",))


@pytest.fixture()
def faked(edited, monkeypatch):
    import gcs_admm_amd.batch
    import gcs_admm_amd.rounding
    _Batch.log = []
    monkeypatch.setattr(gcs_admm_amd.batch, "BatchSolver", _Batch)
    monkeypatch.setattr(gcs_admm_amd.rounding, "rounding_problem", lambda m, As, bs, seed=0: None)
    monkeypatch.setattr(gcs_admm_amd.rounding, "rounding_many", lambda problems, **kw: [(1.0, {}, {}) for _ in problems])
    *_, sq = edited
    c = sq.centers
    yield sq, c[:2], c[-2:]
    sq.close()


def test_without_keep_and_seed_solve_is_called_as_before(faked):
    sq, S, G = faked
    recs = sq.solve(S, G, max_it=7)
    assert _Batch.log == [("init", 2), ("solve", dict(max_it=7)), ("close",)]
    assert all("snapshot" not in r for r in recs)


def test_keep_exports_before_the_batch_is_closed(faked):
    sq, S, G = faked
    recs = sq.solve(S, G, keep=True)
    want = [sq.vertex_ids(r["graph"]).tolist() for r in recs]
    assert _Batch.log == [("init", 2), ("solve", {}), ("export", want), ("close",)]
    assert [r["snapshot"] for r in recs] == [("snapshot", 0), ("snapshot", 1)]


def test_seed_goes_to_the_batch_with_the_ids(faked):
    sq, S, G = faked
    recs = sq.solve(S, G, seed=["a", None], keep=True, rho=2.0)
    (_, kw), = [e for e in _Batch.log if e[0] == "solve"]
    assert kw["seed"] == ["a", None] and kw["rho"] == 2.0
    assert [np.asarray(i).tolist() for i in kw["vertex_ids"]] == [sq.vertex_ids(r["graph"]).tolist() for r in recs]
    _Batch.log.clear()
    with pytest.raises(ValueError, match="one snapshot or None per query"):
        sq.solve(S, G, seed=["a"])
    assert _Batch.log == []                                            # refused before a batch is made


# ------------------------------------------------------------------------------------------- the claim, on the oracle
def test_a_seeded_query_stops_in_half_the_iterations_at_the_same_rounded_cost(oracle_lib):
    scene = R.Scene()
    base = scene.solve(scene.s, scene.t)
    assert base["status"] == 0 and base["iterations"] > 300
    rows = list(R.queries(scene, base))
    assert [label for label, *_ in rows] == ["shift0.05", "shift0.2", "shift0.2-removed3", "shift0.5", "shift0.5-removed6"]
    for label, s, t, removed in rows:
        cold = scene.solve(s, t, removed)
        seeded = scene.solve(s, t, removed, seed=base)
        print(label, "edges", cold["graph"].num_edges, "cold", cold["iterations"], "seeded", seeded["iterations"], "rounded", cold["rounded_cost"],
              seeded["rounded_cost"], "relaxed", cold["cost"], seeded["cost"])
        assert cold["status"] == 0 and seeded["status"] == 0, label
        assert cold["graph"].num_vertices == 42 - len(removed), label
        assert 2 * seeded["iterations"] <= cold["iterations"], (label, seeded["iterations"], cold["iterations"])
        assert abs(seeded["rounded_cost"] - cold["rounded_cost"]) <= 1e-5, (label, seeded["rounded_cost"], cold["rounded_cost"])
