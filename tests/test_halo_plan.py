"""What a vertex partition decides on the host, checked without a GPU: gcs_admm_amd/csrc/halo_plan.h compiled for the host
(tests/hostemu/halo_plan_emu.cpp beside the create-plan shim, same sizing objects).  Pinned here from literal data: every refusal of
gcsadmm_check_halo with its text and the order of the checks, where column j of the send list sits in the packed message (against the
numpy rule of test_partition.py::test_halo_message_layout_over_gloo as well), and which wavefronts the overlapped loop launches as the
boundary.  The last three tests build the header with one seeded error each and require these checks to fail.  What the GPU does with
these plans is checked by test_gpu_configs.py (halo pack / unpack, overlapped against serial, the strips)."""
import ctypes as C

import numpy as np
import pytest

import hostemu_lib as H
import test_create_plan as cp
from gcs_admm_amd.abi import HaloDesc
from gcs_admm_amd.graph import lattice_boxes
from gcs_admm_amd.partition import build_partition, strip_owner
from gcs_admm_amd.solver import halo_arrays
from mutant_build import build_mutants

OK, BAD_ARG = cp.OK, cp.BAD_ARG
WAVES = dict(vertex_program=1)       # every generic vertex on the wavefront program, as test_create_plan.py forces it


def prepare(lib):
    lib.halo_emu_error.restype = C.c_char_p
    return lib


@pytest.fixture(scope="module")
def lib():
    return prepare(H.emu_library("haloplanemu"))


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def desc(peers, send_ptr, send_cols, recv_ptr, recv_cols, num_peers=None):
    """(HaloDesc, arrays it points into); None: a null pointer"""
    keep = [None if a is None else i32(a) for a in (peers, send_ptr, send_cols, recv_ptr, recv_cols)]
    ptr = [None if a is None else a.ctypes.data for a in keep]
    return HaloDesc(len(peers) if num_peers is None else num_peers, *ptr), keep


def set_plan(lib, g, **kw):
    d, keep = cp.descriptor(g, **kw)
    assert lib.halo_emu_plan(C.byref(d)) == OK, lib.halo_emu_error().decode()


def vec(lib, name, cap=4096):
    buf = (C.c_int * cap)()
    n = lib.halo_emu_vec(name.encode(), buf, cap)
    assert 0 <= n <= cap, (name, n)
    return list(buf[:n])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
# rank 0 of a 3 x 2 lattice cut into two strips: 4 vertices, owned columns 0 .. 13, ghost columns 14 .. 23, one peer, 10 cut columns
SEND = [5, 8, 9, 12, 13, 3, 6, 7, 10, 11]
RECV = list(range(14, 24))


def strip_plan(lib):
    g = lattice_boxes(3, 2)
    part = build_partition(g, strip_owner(g, 2), 0, 2)
    assert (int(part.graph.inc_ptr[-1]), part.num_incidences) == (14, 24)
    peers, ptr, sc, rc = halo_arrays(part.send_idx, part.recv_idx)
    assert (list(peers), list(ptr), list(sc), list(rc)) == ([1], [0, 10], SEND, RECV)          # the literals above are this partition's
    set_plan(lib, part.graph, num_incidences=part.num_incidences)


def check(lib, rank, world, d):
    st = lib.halo_emu_check(rank, world, None if d is None else C.byref(d[0]))
    return st, lib.halo_emu_error().decode()


def check_refusals(lib):
    """every refusal, in the order the checks are made; each descriptor also breaks a LATER rule, which must not be the one reported"""
    strip_plan(lib)
    good = lambda: desc([1], [0, 10], SEND, [0, 10], RECV)
    assert check(lib, 0, 2, good()) == (OK, "")
    assert check(lib, 0, 2, desc([], [0], [], [0], [])) == (OK, "")          # no neighbours
    assert check(lib, 0, 2, desc([], None, None, None, None)) == (OK, "")    # ... and then no arrays either
    # bad rank or world, null descriptor (a null array behind it is not looked at)
    null_arrays = desc([1], None, SEND, [0, 10], RECV)
    bad_comm = (BAD_ARG, "bad communicator arguments")
    assert check(lib, 0, 2, None) == bad_comm
    assert check(lib, 0, 0, null_arrays) == bad_comm
    assert check(lib, -1, 2, null_arrays) == bad_comm
    assert check(lib, 2, 2, null_arrays) == bad_comm
    # null array (the totals behind it differ)
    null = (BAD_ARG, "null halo array")
    for k in range(5):
        arrays = [[1], [0, 10], SEND, [0, 9], RECV]
        arrays[k] = None
        assert check(lib, 0, 2, desc(*arrays, num_peers=1)) == null, k
    assert check(lib, 0, 2, desc([1], [0, 10], SEND, [0, 9], RECV, num_peers=-1)) == null
    # send and receive totals differ (the peer is the rank itself)
    assert check(lib, 0, 2, desc([0], [0, 10], SEND, [0, 9], RECV)) == (
        BAD_ARG, "halo lists: a partition sends and receives one column per cut edge and neighbour")
    # per-peer counts differ at equal totals; a negative count; a receive block that does not start where the send block does
    # (each with a peer rank out of range behind it)
    counts = (BAD_ARG, "halo lists: send and receive counts per peer must agree")
    assert check(lib, 0, 3, desc([1, 7], [0, 4, 10], SEND, [0, 6, 10], RECV)) == counts
    assert check(lib, 0, 3, desc([1, 7], [0, 12, 10], SEND, [0, 12, 10], RECV)) == counts
    assert check(lib, 0, 3, desc([7, 1], [0, 5, 10], SEND, [1, 6, 10], RECV)) == counts
    # peer rank: out of range, negative, the rank itself (each with a column out of range behind it); the first peer's rank is
    # reported before the second peer's counts
    peer = (BAD_ARG, "halo lists: bad peer rank")
    far = [99] + SEND[1:]
    assert check(lib, 0, 2, desc([2], [0, 10], far, [0, 10], RECV)) == peer
    assert check(lib, 0, 2, desc([-1], [0, 10], far, [0, 10], RECV)) == peer
    assert check(lib, 0, 2, desc([0], [0, 10], far, [0, 10], RECV)) == peer
    assert check(lib, 1, 2, desc([1], [0, 10], far, [0, 10], RECV)) == peer
    assert check(lib, 0, 4, desc([0, 1, 2], [0, 2, 6, 10], SEND, [0, 2, 5, 10], RECV)) == peer
    assert check(lib, 3, 4, desc([0, 1, 2], [0, 2, 6, 10], SEND, [0, 2, 5, 10], RECV)) == counts
    # column out of range: send, receive, negative (a ghost column sent behind it)
    rng = (BAD_ARG, "halo lists: column out of range")
    assert check(lib, 0, 2, desc([1], [0, 10], SEND[:9] + [24], [0, 10], RECV)) == rng
    assert check(lib, 0, 2, desc([1], [0, 10], SEND, [0, 10], RECV[:9] + [24])) == rng
    assert check(lib, 0, 2, desc([1], [0, 10], [5, -1] + SEND[2:], [0, 10], RECV)) == rng
    assert check(lib, 0, 2, desc([1], [0, 10], [5, 14] + SEND[2:], [0, 10], [-1] + RECV[1:])) == rng          # (entry by entry)
    assert check(lib, 0, 2, desc([1], [0, 10], SEND[:9] + [23], [0, 10], RECV)) != rng          # 23 is the last column
    # a send column that is a ghost column (an owned column received behind it, and in the same entry)
    assert check(lib, 0, 2, desc([1], [0, 10], SEND[:4] + [14] + SEND[5:], [0, 10], RECV[:4] + [13] + RECV[5:])) == (
        BAD_ARG, "halo lists: send column is not an owned incidence")
    # a receive column that is an owned column
    assert check(lib, 0, 2, desc([1], [0, 10], SEND, [0, 10], RECV[:9] + [13])) == (BAD_ARG, "halo lists: receive column is not a ghost column")


def test_every_refusal_in_order(lib):
    check_refusals(lib)


# ---- layout ---------------------------------------------------------------------------------------------------------------------
def layout(lib, c, d):
    n_send = lib.halo_emu_layout(c, C.byref(d[0]))
    got = {k: vec(lib, k) for k in ("peers", "peer_cnt", "peer_off", "send_cols", "base", "stride")}
    got["n_send"], got["n_recv"] = n_send, lib.halo_emu_vec(b"n_recv", None, 0)
    return got


def packed(copy, c, cols, base, stride):
    """halo_pack_kernel: word w of column j of the list goes to base[j] + w stride[j]"""
    buf = np.full(c * len(cols), np.nan)
    for j, col in enumerate(cols):
        for w in range(c):
            buf[base[j] + w * stride[j]] = copy[w, col]
    return buf


def check_layout(lib):
    """base[lo + j] = lo c + j, stride = cnt: per peer one block [c][cnt] at lo c"""
    for c in (3, 5):
        none = layout(lib, c, desc([], [0], [], [0], []))
        assert none == dict(peers=[], peer_cnt=[], peer_off=[], send_cols=[], base=[], stride=[], n_send=0, n_recv=0)
        one = layout(lib, c, desc([4], [0, 4], [9, 2, 7, 5], [0, 4], [20, 21, 22, 23]))
        assert one == dict(peers=[4], peer_cnt=[4], peer_off=[0], send_cols=[9, 2, 7, 5], base=[0, 1, 2, 3], stride=[4, 4, 4, 4], n_send=4, n_recv=4)
        two = layout(lib, c, desc([0, 2], [0, 1, 4], [9, 2, 7, 5], [0, 1, 4], [20, 21, 22, 23]))
        assert two == dict(peers=[0, 2], peer_cnt=[1, 3], peer_off=[0, 1], send_cols=[9, 2, 7, 5], n_send=4, n_recv=4,
                           base={3: [0, 3, 4, 5], 5: [0, 5, 6, 7]}[c], stride=[1, 3, 3, 3])
    # the lists build_partition makes for three strips: the message is test_partition.py's, per peer copy[:, cols of the peer].ravel()
    g = lattice_boxes(3, 6, seed=2)
    owner = strip_owner(g, 3)
    peers_seen = []
    for rank in range(3):
        part = build_partition(g, owner, rank, 3)
        peers, ptr, sc, rc = halo_arrays(part.send_idx, part.recv_idx)
        peers_seen.append(len(peers))
        for c in (3, 5):
            got = layout(lib, c, desc(peers, ptr, sc, ptr, rc))
            assert got["peers"] == list(peers) and got["peer_off"] == list(ptr[:-1]) and got["peer_cnt"] == list(np.diff(ptr))
            assert got["send_cols"] == list(sc) and got["n_send"] == got["n_recv"] == len(sc)
            copy = np.arange(c * part.num_incidences, dtype=np.float64).reshape(c, part.num_incidences)
            want = np.empty(c * len(sc))
            for p in range(len(peers)):
                lo, hi = int(ptr[p]), int(ptr[p + 1])
                want[lo * c:hi * c] = copy[:, sc[lo:hi]].ravel()
            assert np.array_equal(packed(copy, c, sc, got["base"], got["stride"]), want)
            # the receiving side has the same layout: unpacking the peer's block fills the ghost columns in list order
            back = np.zeros_like(copy)
            for j, col in enumerate(rc):
                back[:, col] = want[np.array(got["base"])[j] + np.arange(c) * got["stride"][j]]
            for p in range(len(peers)):
                lo, hi = int(ptr[p]), int(ptr[p + 1])
                assert np.array_equal(back[:, rc[lo:hi]], want[lo * c:hi * c].reshape(c, hi - lo))
    assert peers_seen == [1, 2, 1]


def test_message_layout(lib):
    check_layout(lib)


# ---- overlap split --------------------------------------------------------------------------------------------------------------
# wavefront-program plans of n = 2 lattices: (cells per row, rows, wave_slots) -> wavefronts; vertices 0, 1 are the terminals (closed
# form), the cells follow, 4 columns each from column 4 on
PLANS = {2: (3, 2, 3), 3: (3, 2, 2), 5: (5, 2, 2), 10: (5, 2, 1)}
NO_SPLIT = ([], 0)


def split(lib, cols, mode=0, n_wg=-1, n_split=-1):
    cols = i32(cols)
    b = lib.halo_emu_split(cols.ctypes.data_as(C.c_void_p), len(cols), mode, n_wg, n_split)
    return vec(lib, "ids"), b


def wave_plan(lib, plan_lib, n_waves):
    """sets the plan; the first column of the first and of the last generic vertex, one column per wavefront"""
    nx, ny, slots = PLANS[n_waves]
    g = lattice_boxes(nx, ny)
    set_plan(lib, g, wave_slots=slots, **WAVES)
    p = cp.plan(plan_lib, g, wave_slots=slots, **WAVES)
    w = cp.waves(p)
    assert p.n_waves == n_waves and len(p.wg_vtx) == 0 and w[0][0] == 2 and w[-1][-1] == g.num_vertices - 1
    assert list(g.inc_ptr[:3]) == [0, 2, 4] and np.all(np.diff(g.inc_ptr[2:]) == 4)
    col = lambda v: 4 + 4 * (int(v) - 2)
    return col(w[0][0]), col(w[-1][-1]), [col(ws[0]) for ws in w]


def check_split(lib, plan_lib):
    for n in (2, 3, 5):
        first, last, every = wave_plan(lib, plan_lib, n)
        rest = list(range(n))
        assert split(lib, [first]) == (rest, 1)                                    # boundary first, the interior in ascending order
        assert split(lib, [last]) == ([n - 1] + rest[:-1], 1)
        assert split(lib, [last, first, last + 1]) == (([0, n - 1] + rest[1:-1], 2) if n > 2 else NO_SPLIT)
        assert split(lib, every) == NO_SPLIT                                       # all boundary
        assert split(lib, []) == NO_SPLIT                                          # none boundary
        assert split(lib, [0, 2]) == NO_SPLIT                                      # (the columns of a terminal: no wavefront holds it)
        assert split(lib, [], mode=1) == (rest, 1)                                 # mode 1: max(1, n / 4) wavefronts play the boundary
        assert split(lib, [0], mode=1) == NO_SPLIT                                 # ... only when nothing is sent
        assert split(lib, [last], mode=1) == ([n - 1] + rest[:-1], 1)
        assert split(lib, [first], mode=2) == NO_SPLIT and split(lib, [], mode=2) == NO_SPLIT
        assert split(lib, [first], n_wg=1) == NO_SPLIT and split(lib, [], mode=1, n_wg=1) == NO_SPLIT      # one workgroup-program vertex
        assert split(lib, [first], n_split=1) == NO_SPLIT
    wave_plan(lib, plan_lib, 10)
    assert split(lib, [], mode=1) == (list(range(10)), 2)                          # 10 / 4
    # fewer than two wavefronts
    g = lattice_boxes(3, 1)
    set_plan(lib, g, wave_slots=8, **WAVES)
    assert cp.plan(plan_lib, g, wave_slots=8, **WAVES).n_waves == 1
    assert split(lib, [4]) == NO_SPLIT and split(lib, [], mode=1) == NO_SPLIT
    # a plan of its own with workgroup-program vertices (the automatic choice for a small graph)
    set_plan(lib, lattice_boxes(3, 2))
    assert split(lib, [4]) == NO_SPLIT and split(lib, [], mode=1) == NO_SPLIT


@pytest.fixture(scope="module")
def plan_lib():
    return cp.load(cp.build_lib())


def test_overlap_split(lib, plan_lib):
    check_split(lib, plan_lib)


# ---- the checks have teeth ------------------------------------------------------------------------------------------------------
# (anchor in halo_plan.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "base_without_c": [("H.base[lo + j] = lo * c + j;", "H.base[lo + j] = lo + j;")],
    "peer_may_be_self": [(" || hd->peer_rank[p] == rank)", ")")],
    "quarter_may_be_zero": [("w < std::max(1, n_waves / 4);", "w < n_waves / 4;")],
}


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    *sizes, (source, _) = H.sources(H.LIBRARIES["haloplanemu"][0])
    libs = build_mutants(tmp_path_factory.mktemp("halo_mutants"), "halo_plan.h", MUTANTS, source, flags=[H.INCLUDE], more=sizes)
    return {k: prepare(v) for k, v in libs.items()}


def test_clean_copy_passes(builds, plan_lib):
    check_refusals(builds["clean"]); check_layout(builds["clean"]); check_split(builds["clean"], plan_lib)


@pytest.mark.parametrize("mutant,fails", [("base_without_c", "layout"), ("peer_may_be_self", "refusals"), ("quarter_may_be_zero", "split")])
def test_seeded_error_is_rejected(builds, plan_lib, mutant, fails):
    checks = dict(refusals=lambda l: check_refusals(l), layout=lambda l: check_layout(l), split=lambda l: check_split(l, plan_lib))
    for name, run in checks.items():
        if name == fails:
            with pytest.raises(AssertionError):
                run(builds[mutant])
        else:
            run(builds[mutant])        # the other rules are untouched
