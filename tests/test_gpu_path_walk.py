"""walk_kernel on the device (gcsadmm_walks_* through walks.DeviceWalks) against the rule's Python restatement ``walks.walk_reference``
element for element, the limits and the error paths, and ``SceneQueries.solve(walk="device")`` against ``rounding_members`` on the
mirror.  The same cases go through the host build in test_path_walk.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import walk_cases as WC
from gcs_admm_amd import walks as W
from gcs_admm_amd.abi import GcsAdmmError

pytestmark = pytest.mark.gpu

TORCH = {np.float64: "float64", np.float32: "float32"}


def lists(case):
    return (case.out_ptr, case.out_head, case.out_edge, case.src, case.dst)


def on_device(case, dtype):
    import torch
    return torch.tensor(case.y.astype(dtype), device="cuda:0")


@pytest.mark.parametrize("dtype", WC.DTYPES, ids=["f64", "f32"])
def test_device_equals_the_mirror_one_problem_per_call(oracle_lib, dtype):
    for case in WC.all_cases(oracle_lib):
        with W.DeviceWalks([lists(case)]) as dw:
            y = on_device(case, dtype)
            for seed in WC.SEEDS:
                (paths, status), = dw.sample([y], [seed], 0, WC.WALKS, case.max_len)
                assert len(paths) == WC.WALKS and status.dtype == np.int32
                WC.assert_equals_reference(case, dtype, seed, 0, paths, status)


@pytest.mark.parametrize("dtype", WC.DTYPES, ids=["f64", "f32"])
def test_device_equals_the_mirror_three_problems_per_call(oracle_lib, dtype):
    """problems of different sizes side by side, every one with its own seed; max_len is the call's, so the mirror takes it too"""
    cases = WC.all_cases(oracle_lib)
    for trio in (cases[0:3], cases[3:6], cases[6:9], cases[9:12], cases[11:14]):
        max_len = max(c.V for c in trio)
        with W.DeviceWalks([lists(c) for c in trio]) as dw:
            got = dw.sample([on_device(c, dtype) for c in trio], list(WC.SEEDS), 0, WC.WALKS)
            for c, seed, (paths, status) in zip(trio, WC.SEEDS, got):
                WC.assert_equals_reference(c, dtype, seed, 0, paths, status, max_len)
            # a short max_len for all: the overruns are cut where the mirror cuts them
            got = dw.sample([on_device(c, dtype) for c in trio], list(WC.SEEDS), 0, 4, max_len=3)
            for c, seed, (paths, status) in zip(trio, WC.SEEDS, got):
                WC.assert_equals_reference(c, dtype, seed, 0, paths, status, 3)


def test_walks_are_independent(oracle_lib):
    """sample(0, 16) == sample(0, 8) ++ sample(8, 8), and a problem's walks do not depend on what else is in the call"""
    a, b, c = WC.benchmark(oracle_lib, "benchmark3"), WC.handmade()[0], WC.benchmark(oracle_lib, "benchmark4")
    ys = [on_device(x, np.float64) for x in (a, b, c)]
    seeds = [3, 2 ** 64 - 1, 11]
    same = lambda p, q: len(p[0]) == len(q[0]) and all(np.array_equal(u, v) for u, v in zip(p[0], q[0])) and np.array_equal(p[1], q[1])
    with W.DeviceWalks([lists(x) for x in (a, b, c)]) as dw:
        whole, lo, hi = dw.sample(ys, seeds, 0, 16), dw.sample(ys, seeds, 0, 8), dw.sample(ys, seeds, 8, 8)
    for i in range(3):
        assert same(whole[i], (lo[i][0] + hi[i][0], np.concatenate([lo[i][1], hi[i][1]]))), i
    max_len = max(x.V for x in (a, b, c))
    for i, x in enumerate((a, b, c)):
        with W.DeviceWalks([lists(x)]) as dw:
            assert same(dw.sample([ys[i]], [seeds[i]], 0, 16, max_len)[0], whole[i]), i
        WC.assert_equals_reference(x, np.float64, seeds[i], 0, *whole[i], max_len)


def big_problem(V):
    """src 0, dst 1: 0 -> V - 1 -> 1 (the most probable path) and 0 -> V - 2, which has no way on"""
    out_ptr = np.full(V + 1, 2, np.int32); out_ptr[0] = 0; out_ptr[V] = 3
    return SimpleNamespace(name=f"big{V}", V=V, out_ptr=out_ptr, out_head=np.array([V - 1, V - 2, 1], np.int32), out_edge=np.array([0, 1, 2], np.int32),
                           y=np.array([1.0, 0.5, 1.0]), src=0, dst=1, max_len=4)


def test_the_largest_bitmap():
    import torch
    big = big_problem(W.MAX_VERTICES)
    small = WC.handmade()[2]
    with W.DeviceWalks([lists(small), lists(big)]) as dw:
        ys = [on_device(small, np.float64), on_device(big, np.float64)]
        for _ in range(2):                                     # the second launch finds the bitmap as the first one left it
            got = dw.sample(ys, [1, 2], 0, 12, max_len=4)
            WC.assert_equals_reference(small, np.float64, 1, 0, *got[0], 4)
            WC.assert_equals_reference(big, np.float64, 2, 0, *got[1], 4)
        paths, status = got[1]
        assert paths[0].tolist() == [0, W.MAX_VERTICES - 1, 1] and status[0] == W.OK
        dead = [p.tolist() for p, s in zip(paths, status) if s == W.DEAD_END]
        assert dead and all(p == [0, W.MAX_VERTICES - 2] for p in dead)
        with pytest.raises(GcsAdmmError, match=r"status 2.*problem 1: more than 524288 vertices"):
            W.DeviceWalks([lists(small), lists(big_problem(W.MAX_VERTICES + 1))])
        got = dw.sample(ys, [1, 2], 0, 12, max_len=4)          # the object made before the refusal still serves
        WC.assert_equals_reference(big, np.float64, 2, 0, *got[1], 4)
    torch.cuda.synchronize()


def test_bad_arguments_are_refused_and_the_object_stays_usable():
    import torch
    c, d = WC.handmade()[2], WC.handmade()[5]
    with W.DeviceWalks([lists(c), lists(d)]) as dw:
        ys = [on_device(c, np.float64), on_device(d, np.float64)]

        def still_serves():
            got = dw.sample(ys, [5, 6], 0, 8)
            WC.assert_equals_reference(c, np.float64, 5, 0, *got[0], 4)
            WC.assert_equals_reference(d, np.float64, 6, 0, *got[1], 4)
        still_serves()
        head = c.out_head.copy(); head[2] = c.V
        with pytest.raises(GcsAdmmError, match=r"status 1.*problem 1: head out of range at out-list entry 2"):
            W.DeviceWalks([lists(d), (c.out_ptr, head, c.out_edge, c.src, c.dst)])
        ptr = c.out_ptr.copy(); ptr[1], ptr[2] = ptr[2], ptr[1]
        with pytest.raises(GcsAdmmError, match=r"status 1.*problem 0: out_ptr is not monotone at vertex 1"):
            W.DeviceWalks([(ptr, c.out_head, c.out_edge, c.src, c.dst)])
        with pytest.raises(GcsAdmmError, match=r"status 1.*problem 0: src or dst out of range"):
            W.DeviceWalks([(c.out_ptr, c.out_head, c.out_edge, c.V, c.dst)])
        still_serves()
        with pytest.raises(GcsAdmmError, match=r"status 1.*max_len must be at least 1"):
            dw.sample(ys, [5, 6], 0, 8, max_len=0)
        with pytest.raises(GcsAdmmError, match=r"status 1.*must be non-negative"):
            dw.sample(ys, [5, 6], 0, -1)
        with pytest.raises(GcsAdmmError, match=r"status 1.*must be non-negative"):
            dw.sample(ys, [5, 6], -1, 8)
        with pytest.raises(GcsAdmmError, match=r"status 2.*above 2\^31 - 1"):
            dw.sample(ys, [5, 6], 0, 2 ** 20, max_len=2 ** 11)
        still_serves()
        # a null activation pointer, and a dtype that is neither: the raw call
        seed = np.array([5, 6], np.int64)
        out = np.full(2 * 8 * 4 + 32, -7, np.int32)
        args = lambda ptrs, dtype: (ptrs, dtype, seed.ctypes.data, 0, 8, 4, torch.cuda.current_stream().cuda_stream, out.ctypes.data,
                                    out[64:].ctypes.data, out[80:].ctypes.data)
        with pytest.raises(GcsAdmmError, match=r"status 1.*problem 1: null activations"):
            dw._call("gcsadmm_walks_sample", *args((C.c_void_p * 2)(ys[0].data_ptr(), None), 0))
        with pytest.raises(GcsAdmmError, match=r"status 1.*state_dtype"):
            dw._call("gcsadmm_walks_sample", *args((C.c_void_p * 2)(ys[0].data_ptr(), ys[1].data_ptr()), 2))
        assert np.all(out == -7)                                # a refused call writes nothing
        still_serves()
        # no walks: empty outputs, not an error
        got = dw.sample(ys, [5, 6], 0, 0)
        assert [(len(p), len(s)) for p, s in got] == [(0, 0), (0, 0)]
        # what the Python layer refuses by itself
        with pytest.raises(ValueError, match="one activation tensor and one seed per problem"):
            dw.sample(ys[:1], [5, 6])
        with pytest.raises(ValueError, match="all float64 or all float32"):
            dw.sample([ys[0], ys[1].float()], [5, 6])
        with pytest.raises(ValueError, match="problem 0: the activations must be"):
            dw.sample([ys[0].cpu(), ys[1]], [5, 6])
        with pytest.raises(ValueError, match="problem 1: the activations must be"):
            dw.sample([ys[0], ys[1][:2]], [5, 6])
        still_serves()
    with pytest.raises(GcsAdmmError, match="closed"):
        dw.sample(ys, [5, 6])
    with W.DeviceWalks([]) as none:                             # no problems: an empty call
        assert none.sample([], []) == []
    from gcs_admm_amd import abi
    assert abi.load_library().gcsadmm_walks_sample(None, None, 0, None, 0, 1, 1, None, None, None, None) == 1


# ------------------------------------------------------------------------------------------- end to end
def benchmark1_queries():
    """the three queries of test_gpu_point_locate.py::test_solve_equals_solo_solvers_and_the_reference_record"""
    import locate_cases as L
    from gcs_admm_amd.cases import fixture_sets
    from gcs_admm_amd.graph import _as_box
    As_all, bs_all, n, _, _ = fixture_sets("benchmark1")
    p = lambda k: (np.asarray(bs_all[k])[:n] - np.asarray(bs_all[k])[n:]) / 2
    As, bs, _, _ = L.region_sets("benchmark1")
    keys = list(As)

    def inner(k, f):
        lo, hi = _as_box(np.asarray(As[k], float), np.asarray(bs[k], float))
        return lo + np.asarray(f) * (hi - lo)
    S = np.array([p('s'), inner(keys[0], (0.3, 0.6)), inner(keys[-1], (0.7, 0.2))])
    G = np.array([p('t'), inner(keys[-1], (0.4, 0.4)), inner(keys[1], (0.5, 0.5))])
    return As, bs, n, S, G


def test_solve_with_device_walks(monkeypatch):
    """``walk="device"`` rounds every query exactly as ``rounding_members`` does with the mirror as its sampler, on the host copy of the
    member's activations: the same candidate paths, bit-identical results; the solve itself is that of ``walk="host"`` to the byte"""
    from gcs_admm_amd import SceneQueries, rounding
    from gcs_admm_amd.cases import load_fixture
    As, bs, n, S, G = benchmark1_queries()
    seeds = [0, 4, 9]
    offered = []
    device_solver = rounding.solve_path_restrictions_device

    def recording(As_, bs_, n_, paths, *rest):
        offered[-1].append([list(p) for p in paths])
        return device_solver(As_, bs_, n_, paths, *rest)
    monkeypatch.setattr(rounding, "solve_path_restrictions_device", recording)
    with SceneQueries(As, bs, n) as sq:
        offered.append([])
        dev = sq.solve(S, G, seeds=seeds, return_state=True, walk="device")
        offered.append([])
        host = sq.solve(S, G, seeds=seeds, return_state=True, walk="host")
    # the walk never touches the solve
    for a, b in zip(dev, host):
        assert (a["status"], a["iterations"]) == (b["status"], b["iterations"]) and a["trace"].tobytes() == b["trace"].tobytes()
        assert np.float64(a["cost"]).tobytes() == np.float64(b["cost"]).tobytes()
        assert all(a["state"][k].tobytes() == b["state"][k].tobytes() for k in a["state"])
    members = [SimpleNamespace(zedge=rec["state"]["zedge"]) for rec in dev]
    graphs = [rec["graph"] for rec in dev]
    offered.append([])
    want = rounding.rounding_members(members, graphs, seeds=seeds, sampler=WC.mirror_sampler)
    assert offered[0] == offered[2] and len(offered[0]) >= 1 and all(len(rnd) >= 3 for rnd in offered[0][:1])
    for rec, (cost, x_v, y_v) in zip(dev, want):
        assert np.isfinite(cost) and np.float64(rec["rounded_cost"]).tobytes() == np.float64(cost).tobytes()
        assert rec["y_v_rounded"] == y_v and list(rec["x_v_rounded"]) == list(x_v)
        assert all(np.asarray(rec["x_v_rounded"][v]).tobytes() == np.asarray(x_v[v]).tobytes() for v in x_v)
    # the fixture's own query: the reference's rounded length
    gold = load_fixture("benchmark1")[0]["golden_v3"]
    x, y = dev[0]["x_v_rounded"], dev[0]["y_v_rounded"]
    length = sum(float(np.linalg.norm(np.asarray(x[v])[:n] - np.asarray(x[v])[n:])) for v in x if y[v] == 1)
    gx, gy = np.array(gold["x_v_rounded"]), np.array(gold["y_v_rounded"])
    glen = sum(np.linalg.norm(gx[i][:n] - gx[i][n:]) for i in range(len(gy)) if gy[i] == 1)
    assert abs(length - glen) <= 1e-5 * glen and abs(dev[0]["rounded_cost"] - length) <= 1e-9 * glen
