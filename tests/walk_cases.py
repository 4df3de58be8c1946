"""Cases of the device walk (csrc/path_walk_core.h, gcs_admm_amd/walks.py) shared by its CPU and GPU tests: hand-made graphs that
reach every branch of the rule, the four benchmarks under the oracle's activations, the host build of the kernel, and the mirror's
answers computed once per (case, dtype, seed, walk)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

from gcs_admm_amd import walks as W
from hostemu_lib import emu_library

SEEDS = (0, 7, 2 ** 63 + 5)
WALKS = 21                                   # walks 0 .. 20: what rounding draws with M = 20
DTYPES = (np.float64, np.float32)
FREQ_WEIGHTS = (0.5, 0.25, 0.125, 0.0625, 0.0625)
BENCHMARKS = ("benchmark1", "benchmark2", "benchmark3", "benchmark4")


def from_edges(name, V, edges, y, src, dst, max_len=None):
    """a case from an edge list in ANY order: the out-lists are the stable sort by tail, ``y`` goes by edge id"""
    tail = np.array([e[0] for e in edges], np.int64).reshape(-1)
    head = np.array([e[1] for e in edges], np.int32).reshape(-1)
    order = np.argsort(tail, kind="stable")
    out_ptr = np.zeros(V + 1, np.int64); out_ptr[1:] = np.cumsum(np.bincount(tail, minlength=V))
    return SimpleNamespace(name=name, V=V, out_ptr=out_ptr.astype(np.int32), out_head=np.ascontiguousarray(head[order]),
                           out_edge=order.astype(np.int32), y=np.asarray(y, np.float64), src=src, dst=dst, max_len=max_len or V)


def star(degree=130, seed=1):
    """src -> degree middle vertices -> dst: the source's out-list takes three strides, the last one partial"""
    rng = np.random.default_rng(seed)
    edges = [(0, 1 + k) for k in range(degree)] + [(1 + k, degree + 1) for k in range(degree)]
    return from_edges(f"star{degree}", degree + 2, edges, np.concatenate([rng.uniform(0.0, 1.0, degree), np.ones(degree)]), 0, degree + 1)


def fan(weights=FREQ_WEIGHTS):
    d = len(weights)
    return from_edges(f"fan{d}", d + 2, [(0, 1 + k) for k in range(d)] + [(1 + k, d + 1) for k in range(d)], list(weights) + [1.0] * d, 0, d + 1)


def handmade():
    rng = np.random.default_rng(5)
    shuffled = [(int(a), int(b)) for a in range(12) for b in range(12) if a != b and rng.random() < 0.3]
    shuffled = [shuffled[i] for i in rng.permutation(len(shuffled))]
    chain = [(i, i + 1) for i in range(9)]
    cases = [
        star(),
        fan(),
        # 0 -> 1 -> 2, whose only live out-edges lead back to 0 and 1: a dead end by exclusion; 0 -> 3 = dst succeeds
        from_edges("excluded", 4, [(0, 1), (0, 3), (1, 2), (2, 0), (2, 1)], [0.7, 0.3, 1.0, 1.0, 1.0], 0, 3),
        from_edges("all_zero", 3, [(0, 1), (1, 2)], [0.0, 0.0], 0, 2),
        from_edges("weights", 9, [(0, 1 + k) for k in range(7)] + [(1 + k, 8) for k in range(7)],
                   [2.0 ** -41, 2.0 ** -40, 1.0, 1.0000001, 5.0, -0.1, np.nan] + [1.0] * 7, 0, 8),
        from_edges("tie", 4, [(0, 1), (0, 2), (1, 3), (2, 3)], [0.5, 0.5, 1.0, 1.0], 0, 3),
        from_edges("src_is_dst", 2, [(0, 1), (1, 0)], [1.0, 1.0], 0, 0),
        from_edges("long_chain", 10, chain, [1.0] * 9, 0, 9, max_len=5),
        from_edges("exact_fit", 10, chain, [1.0] * 9, 0, 9, max_len=10),
        from_edges("shuffled", 12, shuffled, rng.uniform(-0.1, 1.0, len(shuffled)), 0, 11),
    ]
    assert not np.array_equal(cases[-1].out_edge, np.arange(len(shuffled)))      # an out_edge that is not the identity
    return cases


_bench = {}


def benchmark(oracle_lib, name):
    """a benchmark's graph with the oracle's activations (restrict_cases.oracle_activations), by edge id; computed once"""
    if name not in _bench:
        import restrict_cases as R
        from gcs_admm_amd.cases import load_fixture
        g = load_fixture(name)[1]
        keys, E, y_e = R.oracle_activations(oracle_lib, name)
        assert keys == g.keys and E == g.edges_as_keys()
        out_ptr, out_head, out_edge = W.out_lists(g)
        _bench[name] = SimpleNamespace(name=name, V=g.num_vertices, out_ptr=out_ptr, out_head=out_head, out_edge=out_edge,
                                       y=np.array([y_e[e] for e in E]), src=g.src, dst=g.dst, max_len=g.num_vertices, graph=g, y_e=y_e)
    return _bench[name]


def all_cases(oracle_lib):
    return handmade() + [benchmark(oracle_lib, name) for name in BENCHMARKS]


# ---- the mirror, once per (case, dtype, seed, walk) ----
_ref = {}


def reference(case, dtype, seed, walk, max_len=None):
    max_len = max_len or case.max_len
    key = (case.name, np.dtype(dtype).name, seed, walk, max_len)
    if key not in _ref:
        _ref[key] = W.walk_reference(case.out_ptr, case.out_head, case.out_edge, case.y.astype(dtype), case.src, case.dst, seed, walk, max_len)
    return _ref[key]


def mirror_sampler(members, graphs, seeds, count):
    """the sampler of ``rounding_members`` on ``walk_reference``: reads a host copy of every member's activation row"""
    out = []
    for m, g, seed in zip(members, graphs, seeds):
        y = m.zedge[2 * g.n]
        y = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
        lists = W.out_lists(g)
        got = [W.walk_reference(*lists, y, g.src, g.dst, seed, w, g.num_vertices) for w in range(count)]
        out.append(([p for p, _ in got], np.array([s for _, s in got], np.int32)))
    return out


# ---- the host build of the kernel ----
_lib = []


def emu():
    if not _lib:
        lib = emu_library("walkemu")
        lib.walk_emu_sample.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_uint64] + [C.c_int] * 3 + [C.c_void_p] * 3
        for f, args in ((lib.walk_emu_weight, [C.c_double]), (lib.walk_emu_mix, [C.c_uint64, C.c_uint32, C.c_uint32]), (lib.walk_emu_mulhi, [C.c_uint64] * 2)):
            f.argtypes, f.restype = args, C.c_uint64
        _lib.append(lib)
    return _lib[0]


def emu_sample(case, dtype, seed, first, count, max_len=None):
    """(return code, paths, status) of the host build for walks first .. first + count - 1"""
    max_len = max_len or case.max_len
    y = np.ascontiguousarray(case.y.astype(dtype))
    vtx = np.full((count, max_len), -7, np.int32); length = np.full(count, -7, np.int32); status = np.full(count, -7, np.int32)
    rc = emu().walk_emu_sample(case.V, len(case.out_head), case.out_ptr.ctypes.data, case.out_head.ctypes.data, case.out_edge.ctypes.data,
                               y.ctypes.data, int(np.dtype(dtype) == np.float32), case.src, case.dst, seed % 2 ** 64, first, count, max_len,
                               vtx.ctypes.data, length.ctypes.data, status.ctypes.data)
    return rc, [vtx[w, :max(length[w], 0)] for w in range(count)], status


def assert_equals_reference(case, dtype, seed, first, paths, status, max_len=None):
    """element for element: paths (and with them the lengths) and statuses"""
    for i, (p, s) in enumerate(zip(paths, status)):
        want_p, want_s = reference(case, dtype, seed, first + i, max_len)
        assert s == want_s and np.asarray(p).dtype == np.int32 and np.array_equal(p, want_p), (case.name, np.dtype(dtype).name, seed, first + i, p, s, want_p, want_s)
