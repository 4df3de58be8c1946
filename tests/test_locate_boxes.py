"""The classification of (box, region) pairs and the hit list of gcsadmm_scene_locate_boxes, checked on the host build of the shared
functions (csrc/box_locate_core.h, run lane by lane by tests/hostemu/locate_box_emu.cpp; the kernel is held to this build byte for byte
by test_gpu_locate_boxes.py).  The references are ``graph.polytopes_overlap`` and ``graph.graph_from_sets``: no OUT verdict on a pair
that overlaps, every IN verdict an overlap, and with the UNDECIDED pairs decided by ``polytopes_overlap`` the regions of a box are
exactly the terminal's edges in the graph ``graph_from_sets`` makes.  UNDECIDED is not a place to hide: a box well inside a region
comes back IN.  No GPU."""
import numpy as np
import pytest

import locate_box_cases as bxc
import locate_cases as lc
from gcs_admm_amd.graph import graph_from_sets, polytopes_overlap

OUT, IN, UNDECIDED = lc.OUT, lc.IN, lc.UNDECIDED


def overlaps(polys, lo, hi, n):
    """[Q, P] bool: polytopes_overlap(box, region).  A region lies inside its own box rows, so a pair whose boxes are 1e-6 apart in
    some coordinate is answered without the LP."""
    out = np.zeros((len(lo), len(polys)), bool)
    for r, (A, b) in enumerate(polys):
        rl, rh = bxc.region_box(A, b, n)
        for q in range(len(lo)):
            if np.any(lo[q] > rh + 1e-6) or np.any(hi[q] < rl - 1e-6):
                continue
            out[q, r] = polytopes_overlap(*bxc.box_polytope(lo[q], hi[q]), A, b)
    return out


def test_chunk_is_the_point_kernels():
    assert bxc.emu().locate_box_emu_chunk() == lc.CHUNK


def test_crafted_boxes():
    """a box touching a facet and one touching a vertex (UNDECIDED, overlapping), a gap of 1e-6 (OUT), a box that contains a whole
    region whose centre it misses (UNDECIDED, overlapping), the acute vertex (UNDECIDED, apart), a box 1e-4 wide and one that covers
    everything"""
    names, polys, lo, hi, expect, overlap = bxc.crafted()
    M = lc.dense(bxc.emu_locate_boxes(polys, lo, hi), len(lo), len(polys))
    for (q, name), cls in expect.items():
        assert M[q, names.index(name)] == cls, (q, name, int(M[q, names.index(name)]), cls)
    for (q, name), want in overlap.items():
        A, b = polys[names.index(name)]
        assert polytopes_overlap(*bxc.box_polytope(lo[q], hi[q]), A, b) == want, (q, name)
        assert want or M[q, names.index(name)] != IN
        assert not want or M[q, names.index(name)] != OUT


@pytest.mark.parametrize("n", lc.DIMS)
@pytest.mark.parametrize("kind,offset", lc.FAMILIES)
def test_sound_against_polytopes_overlap(kind, offset, n):
    """40 regions, 12 boxes from 1e-4 to several regions wide: no OUT where box and region overlap, every IN an overlap, and IN plus
    the UNDECIDED pairs that overlap is the overlap relation itself"""
    P, Q = 40, 12
    polys = lc.regions(kind, n, P, offset)
    lo, hi = bxc.boxes(kind, n, P, offset, Q)
    assert (hi - lo).min() < 1.1e-4 and (hi - lo).max() > 3.9
    M = lc.dense(bxc.emu_locate_boxes(polys, lo, hi), Q, P)
    O = overlaps(polys, lo, hi, n)
    assert not np.any((M == OUT) & O), np.argwhere((M == OUT) & O)
    assert not np.any((M == IN) & ~O), np.argwhere((M == IN) & ~O)
    assert np.array_equal((M == IN) | ((M == UNDECIDED) & O), O)
    assert O.any() and (M == UNDECIDED).any() and (M == OUT).any()


@pytest.mark.parametrize("n", lc.DIMS)
@pytest.mark.parametrize("kind", lc.KINDS)
def test_final_sets_equal_graph_from_sets(kind, n):
    """the regions of a box -- IN, or UNDECIDED and then decided by polytopes_overlap -- are the edges of the terminal 's' in the
    graph graph_from_sets makes of {'s': box, 't': a point far away, regions}, in both directions, exactly"""
    P, Q = 10, 6
    polys = lc.regions(kind, n, P, 0.0)
    lo, hi = bxc.boxes(kind, n, P, 0.0, Q)
    ptr, region, cls = bxc.emu_locate_boxes(polys, lo, hi)
    met = 0
    for q in range(Q):
        As, bs = {'s': None, 't': None}, {}
        As['s'], bs['s'] = bxc.box_polytope(lo[q], hi[q])
        As['t'], bs['t'] = bxc.box_polytope(np.full(n, 900.0), np.full(n, 900.0 + 2e-6))
        for r, (A, b) in enumerate(polys):
            As[r], bs[r] = A, b
        g = graph_from_sets(As, bs, n)
        want = sorted(int(g.keys[h]) for t, h in zip(g.edge_tail, g.edge_head) if t == g.src)
        assert want == sorted(int(g.keys[t]) for t, h in zip(g.edge_tail, g.edge_head) if h == g.src)
        hits = range(int(ptr[q]), int(ptr[q + 1]))
        got = [int(region[k]) for k in hits
               if cls[k] == IN or polytopes_overlap(As['s'], bs['s'], *polys[int(region[k])])]
        assert got == want, (q, got, want)
        met += len(want)
    assert met > 0


@pytest.mark.parametrize("n", lc.DIMS)
@pytest.mark.parametrize("kind,offset", lc.FAMILIES)
@pytest.mark.parametrize("P", lc.SIZES)
def test_list_equals_the_plain_double_loop(kind, offset, n, P):
    """hit_ptr, the regions and the classes, through chunks, strides, ballots and the scan, equal a loop over boxes, then regions that
    classifies pair by pair -- one region, around a stride, and into a third and fourth chunk"""
    Q = 3 if P > 200 else 5
    polys = lc.regions(kind, n, P, offset)
    lo, hi = bxc.boxes(kind, n, P, offset, Q)
    got, want = bxc.emu_locate_boxes(polys, lo, hi), bxc.double_loop(polys, lo, hi)
    lc.dense(got, Q, P)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("n", lc.DIMS)
@pytest.mark.parametrize("kind,offset", lc.FAMILIES)
def test_a_box_well_inside_a_region_is_in(kind, offset, n):
    """one box per region, every point of it at least half a region radius from every facet (checked here in numpy at the box's
    corners' worst case): its region comes back IN, not UNDECIDED"""
    P = 65
    polys = lc.regions(kind, n, P, offset)
    lo, hi, rad = bxc.interior_boxes(polys, n)
    for (A, b), l, h, r in zip(polys, lo, hi, rad):
        c, t = 0.5 * (l + h), 0.5 * (h - l)
        worst = (b - A @ c - np.abs(A) @ t) / np.linalg.norm(A, axis=1)        # the least distance of a point of the box to each facet
        assert worst.min() >= 0.5 * r > 0
    M = lc.dense(bxc.emu_locate_boxes(polys, lo, hi), P, P)
    assert np.all(np.diag(M) == IN), np.flatnonzero(np.diag(M) != IN)


def test_zero_boxes_and_zero_regions():
    polys = lc.regions("boxes", 2, 5, 0.0)
    ptr, region, cls = bxc.emu_locate_boxes(polys, np.zeros((0, 2)), np.zeros((0, 2)))
    assert ptr.tolist() == [0] and len(region) == len(cls) == 0
    ptr, region, cls = bxc.emu_locate_boxes([], np.zeros((2, 2)), np.ones((2, 2)), n=2)
    assert ptr.tolist() == [0, 0, 0] and len(region) == 0


def test_a_degenerate_box_is_the_point_rule_with_eps_zero():
    """lo == hi: the box classifier and the point classifier with eps = 0 see the same margins and list the same regions with the
    same classes"""
    for n in lc.DIMS:
        polys = lc.regions("polytopes", n, 130, 0.0)
        pts = lc.points("polytopes", n, 130, 0.0, 20)
        a = bxc.emu_locate_boxes(polys, pts, pts)
        b = lc.emu_locate(polys, pts, eps=0.0)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
