"""One launch per iteration on small graphs (gcsadmm_set_fused_tail, csrc/vertex_wg_kernel.h FUSED TAIL): the last vertex workgroup to
finish runs the edge and control steps.  The solves do not depend on which workgroup runs the edge step, and the tail is edge_kernel's
MODE 1 body in MODE 1's order, so one handle run both ways -- reset, set_fused_tail(0), enqueue(k); reset, set_fused_tail(1),
enqueue(k) -- must leave the same BYTES: the state (copy, mu, zedge, xv, zv, yv), the k trace rows and every field of the control
block.  No tolerance: any difference is a bug (a stale copy read by the tail, a barrier not reached, a sum taken in another order).

The ABI has no reader for the handle's arrival counter; that the tail leaves it at 0 is checked by what follows from it: after a run
that stops inside its span, the same handle reset and run again reproduces the first run bit for bit (with a counter left at c != 0 no
workgroup of the next launch, or the wrong one, would find itself last, and the iteration count would not advance)."""
import ctypes as C

import numpy as np
import pytest

from conftest import interval_chain
from fused_tail_cases import largest_fused_lattice, path3, smallest_unfused_lattice

pytestmark = pytest.mark.gpu


def _solver(g, **kw):
    from gcs_admm_amd.solver import DeviceSolver
    return DeviceSolver(g, **kw)


def _snapshot(s, k):
    s.torch.cuda.synchronize(s.device)
    cb = s.read_control()
    out = {name: getattr(s, name).cpu().numpy().copy() for name in ("copy", "mu", "zedge", "xv", "zv", "yv")}
    out["trace"] = s.trace[:k].cpu().numpy().copy()
    out["cb"] = np.frombuffer(bytes(cb), dtype=np.uint8).copy()
    return out, cb


def _run(s, mode, k, **params):
    s.reset(**params)
    fused = s.set_fused_tail(mode)
    s.enqueue(k)
    snap, cb = _snapshot(s, min(k, s.params.max_it))
    return snap, cb, fused


def _same(a, b, what=""):
    for name in a:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, (what, name)
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), (what, name)


def _both_ways(g, k, params=None, **kw):
    s = _solver(g, **kw)
    try:
        two, cb2, f0 = _run(s, 0, k, **(params or {}))
        one, cb1, f1 = _run(s, 1, k, **(params or {}))
        assert not f0 and f1, "the handle was expected to fuse in mode 1 and not in mode 0"
        assert cb2.it > 1 and np.isfinite(two["copy"]).all() and np.abs(two["copy"]).max() > 0      # the run did something
        _same(two, one, "fused against two launches")
        assert (cb1.it, cb1.status, cb1.inner_iters, cb1.inner_failures) == (cb2.it, cb2.status, cb2.inner_iters, cb2.inner_failures)
        return s, two, cb2
    except Exception:
        s.close()
        raise


def test_path_one_generic_vertex():
    """s, one box, t: two arrivals, one of them a workgroup that holds only closed-form vertices"""
    s, _, cb = _both_ways(path3(), 10)
    assert s.query()["num_workgroup_vertices"] == 1 and s.query()["num_special"] == 2
    s.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("program", ["auto", "workgroup256"])
def test_lattice_rho_changes_inside_the_span(dtype, program):
    """3 x 3 lattice from the zero state, 40 iterations in which rho changes, so that mu_scale != 1 passes through the tail.  With the
    default parameters this lattice reaches its stop test at iteration 79 without one change of rho (CPU oracle), and a longer span
    cannot help; so the adaptation is made eager (nu = 1.5) with tau = 3: rho moves from iteration 3 on, up and down, and mu_scale
    takes the values 3 and 1/3, which are no powers of two (the dual update's separately rounded product matters).
    512 threads (auto: half the workgroup idles in the tail) and 256 (every thread is an edge thread)."""
    from gcs_admm_amd.graph import lattice_boxes
    s, two, _ = _both_ways(lattice_boxes(3, 3), 40, params=dict(nu=1.5, tau_incr=3.0, tau_decr=3.0), state_dtype=dtype, program=program)
    rho = two["trace"][:, 0]
    assert rho.min() != rho.max(), "rho never changed inside the span"
    assert len(set(rho.tolist())) >= 3
    s.close()


@pytest.mark.parametrize("n", [1, 3, 6])
def test_other_dimensions(n):
    """n = 3 and 6 (the BOX instantiations, C = 7 and 13 words per copy: the tail takes them in groups) and n = 1 (the second object)"""
    from gcs_admm_amd.graph import graph_from_sets, lattice_boxes
    g = graph_from_sets(*interval_chain(6)) if n == 1 else lattice_boxes(2, 3, n=n)
    s, _, _ = _both_ways(g, 15)
    s.close()


def test_benchmark4_cold():
    """the headline fixture from the zero state: cold solves, 40 workgroups over the eight XCDs"""
    from gcs_admm_amd.cases import load_fixture
    _, g = load_fixture("benchmark4")
    s, _, _ = _both_ways(g, 30)
    s.close()


def test_last_edge_thread():
    """the largest lattice whose edges fit one edge workgroup (256 edges)"""
    g = largest_fused_lattice()
    assert g.num_edges == 256
    s, _, _ = _both_ways(g, 8)
    s.close()


def test_stop_inside_the_span_and_rerun():
    """max_it = 7 with 12 iterations enqueued: the status leaves RUNNING at iteration 7, the remaining launches change nothing, and the
    handle is left ready -- a second reset + enqueue(12) reproduces the first bit for bit (the arrival counter was left at 0)"""
    from gcs_admm_amd.graph import lattice_boxes
    from gcs_admm_amd.solver import MAX_IT, RUNNING
    s, two, cb = _both_ways(lattice_boxes(3, 3), 12, params=dict(max_it=7))
    assert cb.status == MAX_IT and cb.status != RUNNING and cb.it == 8
    again, cb_again, fused = _run(s, 1, 12, max_it=7)
    assert fused
    _same(two, again, "second fused run after a stop")
    assert (cb_again.it, cb_again.status) == (cb.it, cb.status)
    s.close()


def test_repeats_are_identical():
    """the order of arrival must not matter: two fused runs of benchmark4 leave the same bytes"""
    from gcs_admm_amd.cases import load_fixture
    _, g = load_fixture("benchmark4")
    s = _solver(g)
    a, _, fa = _run(s, 1, 20)
    b, _, fb = _run(s, 1, 20)
    assert fa and fb
    _same(a, b, "fused repeat")
    s.close()


def test_larger_graph_does_not_fuse():
    """more than 256 edges: set_fused_tail reports "not fused" in either mode and the run is the two-launch run"""
    g = smallest_unfused_lattice()
    s = _solver(g)
    two, _, f0 = _run(s, 0, 6)
    one, _, f1 = _run(s, 1, 6)
    assert not f0 and not f1
    _same(two, one, "unfused handle")
    s.close()
