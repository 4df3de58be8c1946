"""Edits of a decided scene, the parts that need no GPU: the host build of the edit kernels (tests/hostemu/scene_edit_emu.cpp compiles
csrc/scene_edit_core.h, the code the kernels run, with the threads one after the other) against ``scene.candidate_pairs`` on the edited
boxes element for element, with the resident pairs' flags and statuses carried; and ``SceneQueries.add_regions`` / ``remove_regions`` on
a stand-in scene against a new object on the edited sets.  The kernels themselves: test_gpu_scene_edit.py."""
import ctypes as C

import numpy as np
import pytest

import locate_cases as L
import scene_edit_cases as E
import sweep_cases as S
from gcs_admm_amd import graph as gr
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError
from gcs_admm_amd.graph import bounding_box, chebyshev_center, polytopes_overlap


@pytest.fixture(scope="module")
def emu():
    return E.load_edit_emu()


def _add(emu, lo, hi, P, pad):
    resident = E.tagged_pairs(lo[:P], hi[:P], pad)
    got, num_new = E.emu_add(emu, lo, hi, P, pad, resident)
    E.check_added(got, num_new, lo, hi, P, pad, resident)
    return resident, got


# ------------------------------------------------------------------------------------------- add
@pytest.mark.parametrize("K", E.APPENDED)
@pytest.mark.parametrize("P", E.RESIDENT)
@pytest.mark.parametrize("n", E.DIMS)
def test_add_equals_candidate_pairs_on_all_boxes(emu, n, P, K):
    for boxes in (E.lattice_boxes, E.random_boxes):
        lo, hi = boxes(n, P + K)
        for pad in S.pads():
            _, got = _add(emu, lo, hi, P, pad)
        if boxes is E.lattice_boxes and P + K >= 3 and K:
            assert len(got[0]) > 0                     # neighbours on the lattice touch: there is something to merge


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("pad_index", [0, 1])
def test_add_on_ties_infinities_and_touching_boxes_across_the_split(emu, pad_index, which):
    pad = S.pads()[pad_index]
    lo, hi, P = E.extras_split(pad, which)
    _, (pa, pb, _, _) = _add(emu, lo, hi, P, pad)
    assert set(zip(pa.tolist(), pb.tolist())) == S.brute_force(lo, hi, pad)
    assert np.sum((lo[:P, 0] == 0.0)) >= 3 and np.sum(lo[P:, 0] == 0.0) >= 3          # ties of the sort key on both sides
    side = slice(0, P) if which == 0 else slice(P, None)                             # the opened sides: resident, then appended
    assert np.isinf(lo[side]).sum() >= 3 and np.isinf(hi[side]).sum() >= 2
    # an appended box with the key of a resident one sorts behind it whatever their order in the arrays: both orders of one tie
    lo2, hi2 = lo.copy(), hi.copy()
    i, j = np.nonzero(lo[:P, 0] == 0.0)[0][0], P + np.nonzero(lo[P:, 0] == 0.0)[0][0]
    lo2[[i, j]], hi2[[i, j]] = lo[[j, i]], hi[[j, i]]
    _add(emu, lo2, hi2, P, pad)


def test_add_nothing_and_everything(emu):
    lo = np.arange(130, dtype=float)[:, None] * np.array([[2.0, 0.0]]); hi = lo + 1.0        # 130 disjoint boxes in a row
    _, got = _add(emu, lo, hi, 65, S.pads()[1])
    assert len(got[0]) == 0
    lo = np.zeros((330, 3)); hi = np.ones((330, 3))                                          # 330 identical boxes: every pair
    _, (pa, pb, _, _) = _add(emu, lo, hi, 200, 0.0)
    ta, tb = np.triu_indices(330, 1)
    assert np.array_equal(pa, ta) and np.array_equal(pb, tb)


# ------------------------------------------------------------------------------------------- remove
def _isolated(n, P):
    """random boxes with one far from all others: box P // 2 has no pairs"""
    lo, hi = E.random_boxes(n, P)
    lo[P // 2] += 1e3; hi[P // 2] += 1e3
    return lo, hi


REMOVALS = {"none": lambda P: [], "all": lambda P: list(range(P))[::-1], "first": lambda P: [0], "last": lambda P: [P - 1],
            "every_second": lambda P: list(range(0, P, 2)), "without_pairs": lambda P: [P // 2]}


@pytest.mark.parametrize("what", sorted(REMOVALS))
@pytest.mark.parametrize("n", E.DIMS)
def test_remove_equals_candidate_pairs_on_the_remaining_boxes(emu, n, what):
    for P in (1, 65, 200):
        lo, hi = _isolated(n, P)
        regions = REMOVALS[what](P)
        for pad in S.pads():
            resident = E.tagged_pairs(lo, hi, pad)
            if what == "without_pairs":
                assert P // 2 not in set(resident[0].tolist()) | set(resident[1].tolist())
            newidx, got = E.emu_remove(emu, lo, hi, pad, regions, resident)
            E.check_removed(newidx, got, lo, hi, pad, regions, resident)
            if what == "none":
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, resident))


def test_remove_refuses_bad_indices(emu):
    lo, hi = E.random_boxes(2, 10)
    resident = E.tagged_pairs(lo, hi, 0.0)
    for regions in ([10], [-1], [3, 3], [0, 9, 0]):
        assert E.emu_remove(emu, lo, hi, 0.0, regions, resident) is None
    assert E.emu_remove(emu, lo, hi, 0.0, [9, 0], resident) is not None


@pytest.mark.parametrize("n", E.DIMS)
def test_add_then_remove_gives_the_list_back(emu, n):
    for boxes in (E.lattice_boxes, E.random_boxes):
        lo, hi = boxes(n, 195)
        P, pad = 65, S.pads()[1]
        resident, got = _add(emu, lo, hi, P, pad)
        newidx, back = E.emu_remove(emu, lo, hi, pad, np.arange(P, 195), got)
        assert np.array_equal(newidx[:P], np.arange(P)) and np.all(newidx[P:] == -1)
        assert len(resident[0]) > 0
        for a, b in zip(back, resident):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_scan_reports_a_total_beyond_int32_without_overflow(emu):
    count = np.full(70000, 69999, np.int32)
    offset = np.empty(70001, np.int64)
    assert emu.edit_emu_scan(count.ctypes.data, 70000, offset.ctypes.data) == 0
    assert offset[-1] == 70000 * 69999 > 2 ** 31 - 1
    assert np.array_equal(offset, np.arange(70001, dtype=np.int64) * 69999)
    count[:] = 30000                                                                         # 2.1e9: just inside
    assert emu.edit_emu_scan(count.ctypes.data, 70000, offset.ctypes.data) == 1 and offset[-1] == 2_100_000_000
    assert emu.edit_emu_scan(None, 0, offset.ctypes.data) == 1 and offset[0] == 0
    new = C.c_longlong(0)
    assert emu.edit_emu_add(9, 0, 0, None, None, 0.0, 0, None, None, None, None, None, None, None, None, 0, C.addressof(new)) == -99


# ------------------------------------------------------------------------------------------- SceneQueries on a stand-in scene
def _sig(poly):
    return np.asarray(poly[0], float).tobytes() + np.asarray(poly[1], float).tobytes()


class FakeEditScene:
    """the interface of scene.DeviceScene that ``SceneQueries`` uses, edits included, in numpy: centres and boxes from the host LPs of
    ``gcs_admm_amd.graph``, the pair list from ``scene.candidate_pairs``, the decisions from ``graph.polytopes_overlap``, ``locate``
    from the host build.  ``undecided``: pairs (two signatures) whose LP reports status -1 with the wrong flag; ``bad``: signature ->
    "center" (the centre LP reports -1) or "flat" (radius 0)."""

    def __init__(self, polys, undecided=(), bad=None):
        self.polys, self.n = list(polys), polys[0][0].shape[1]
        self.undecided, self.bad = {frozenset(p) for p in undecided}, bad or {}
        self.calls, self.closed = [], False

    def _centres(self, polys):
        cen = np.stack([chebyshev_center(A, b) for A, b in polys]).reshape(len(polys), self.n)
        st = np.array([-1 if self.bad.get(_sig(p)) == "center" else 0 for p in polys], np.int32)
        rad = np.array([0.0 if self.bad.get(_sig(p)) == "flat" else 1.0 for p in polys])
        return cen, rad, st

    def _boxes(self):
        bx = [bounding_box(A, b) for A, b in self.polys]
        return np.array([l for l, _ in bx]).reshape(-1, self.n), np.array([h for _, h in bx]).reshape(-1, self.n)

    def _decide(self, pa, pb):
        flags = np.array([1 if polytopes_overlap(*self.polys[a], *self.polys[b]) else 0 for a, b in zip(pa, pb)], np.uint8)
        st = np.zeros(len(pa), np.int32)
        for t, (a, b) in enumerate(zip(pa, pb)):
            if frozenset((_sig(self.polys[a]), _sig(self.polys[b]))) in self.undecided:
                st[t] = -1; flags[t] = 1 - flags[t]
        return flags, st

    def centers(self):
        self.calls.append("centers")
        return self._centres(self.polys)

    def bounds(self):
        self.calls.append("bounds")
        lo, hi = self._boxes()
        return lo, hi, np.zeros((len(self.polys), 2 * self.n), np.int32)

    def candidate_pairs(self, pad=sc.SWEEP_PAD):
        self.calls.append("candidate_pairs")
        self.pa, self.pb = sc.candidate_pairs(*self._boxes(), pad)
        return len(self.pa)

    def overlaps(self, tol):
        self.calls.append("overlaps")
        self.flags, self.st = self._decide(self.pa, self.pb)
        return int(self.flags.sum()), int((self.st < 0).sum())

    def pairs(self):
        return self.pa, self.pb, self.flags, self.st

    def locate(self, pts, eps=L.EPS, tol=L.TOL):
        return L.emu_locate(self.polys, pts, eps, tol, n=self.n)

    def add_regions(self, polys, pad=sc.SWEEP_PAD, tol=1e-9):
        self.calls.append("add_regions")
        cen, rad, st = self._centres(polys)
        if np.any(st < 0) or np.any(rad <= 0):
            e = GcsAdmmError("gcsadmm_scene_add_regions: refused (status 1)")
            e.results = (cen, rad, st)
            raise e
        P = len(self.polys)
        had = {(a, b): (f, s) for a, b, f, s in zip(self.pa.tolist(), self.pb.tolist(), self.flags.tolist(), self.st.tolist())}
        self.polys = self.polys + list(polys)
        self.pa, self.pb = sc.candidate_pairs(*self._boxes(), pad)
        new = self.pb >= P
        self.flags, self.st = self._decide(np.where(new, self.pa, 0), np.where(new, self.pb, 0))
        for t in np.nonzero(~new)[0]:
            self.flags[t], self.st[t] = had[(int(self.pa[t]), int(self.pb[t]))]
        return cen, rad, st, dict(new_pairs=int(new.sum()), overlapping=int(self.flags[new].sum()), undecided=int((self.st[new] < 0).sum()))

    def remove_regions(self, indices):
        self.calls.append("remove_regions")
        stays = np.ones(len(self.polys), bool); stays[np.asarray(indices, int)] = False
        newidx = np.cumsum(stays) - 1
        keep = stays[self.pa] & stays[self.pb]
        self.pa, self.pb = newidx[self.pa[keep]].astype(np.int32), newidx[self.pb[keep]].astype(np.int32)
        self.flags, self.st = self.flags[keep], self.st[keep]
        self.polys = [p for p, s in zip(self.polys, stays) if s]
        return len(self.pa)

    def close(self):
        self.closed = True


def _regions(name):
    """the regions of a committed case; "test1" has a single one: it comes first, and seven of benchmark4 (same plane) under keys of
    their own follow, so that the edits start from a scene of one region"""
    As, bs, n, _ = L.region_sets(name)
    As, bs = dict(As), dict(bs)
    if name == "test1":
        Bs, cs, m, _ = L.region_sets("benchmark4")
        assert len(As) == 1 and m == n
        for k in list(Bs)[:7]:
            As[("benchmark4", k)], bs[("benchmark4", k)] = Bs[k], cs[k]
    return {k: np.asarray(As[k], float) for k in As}, {k: np.asarray(bs[k], float).ravel() for k in bs}, n


def _queries(As, bs, n, keys, **fake):
    from gcs_admm_amd.queries import SceneQueries
    A = {k: As[k] for k in keys}; b = {k: bs[k] for k in keys}
    return SceneQueries(A, b, n, scene=FakeEditScene([(A[k], b[k]) for k in keys], **fake), pair_lp=L.PairLP())


GRAPH_INTS = ("edge_tail", "edge_head", "inc_ptr", "inc_edge", "inc_out", "edge_inc_tail", "edge_inc_head", "poly_ptr")


def _same_object(sq, ref):
    assert sq.keys == ref.keys and len(sq.polys) == len(ref.polys)
    assert all(_sig(p) == _sig(q) for p, q in zip(sq.polys, ref.polys))
    assert sq.centers.tobytes() == ref.centers.tobytes() and sq.centers.shape == ref.centers.shape
    for f in ("edge_tail", "edge_head"):
        assert getattr(sq, f).dtype == getattr(ref, f).dtype == np.int32 and np.array_equal(getattr(sq, f), getattr(ref, f)), f
    assert sq.stats["candidate_pairs"] == ref.stats["candidate_pairs"]
    assert sq.stats["overlaps_redone_on_host"] == ref.stats["overlaps_redone_on_host"]
    rng = np.random.default_rng(len(sq.keys))
    pts = ref.centers[rng.permutation(len(ref.keys))[:4]]           # the centres of four regions as starts and goals
    for g, h in zip(sq.graphs(pts[:2], pts[2:]), ref.graphs(pts[:2], pts[2:])):
        assert g.keys == h.keys
        for f in GRAPH_INTS:
            assert np.array_equal(getattr(g, f), getattr(h, f)), f
        assert g.poly_A.tobytes() == h.poly_A.tobytes() and g.poly_b.tobytes() == h.poly_b.tobytes() and g.interior.tobytes() == h.interior.tobytes()


@pytest.mark.parametrize("name", ["test1", "benchmark4"])
def test_scene_queries_edits_equal_a_new_object(name):
    As, bs, n = _regions(name)
    keys = list(As)
    assert len(keys) >= 8
    now = keys[:-5] if name != "test1" else keys[:1]
    sq = _queries(As, bs, n, now)
    steps = [("add", keys[len(now):-3]), ("add", keys[-3:]), ("remove", [keys[1], keys[-2]]), ("add", [keys[-2]]), ("remove", [keys[0]]),
             ("add", [keys[1], keys[0]])]
    for what, ks in steps:
        if what == "add":
            sq.add_regions({k: As[k] for k in ks}, {k: bs[k] for k in ks})
            now = now + ks
            assert sq.stats["edit_centre_lps"] == len(ks) and sq.stats["edit_bound_lps"] == 2 * n * len(ks)
            assert sq.stats["edit_pair_lps"] == int((sq._pairs["pb"] >= len(now) - len(ks)).sum())
        else:
            sq.remove_regions(ks)
            now = [k for k in now if k not in ks]
            assert sq.stats["edit_centre_lps"] == sq.stats["edit_bound_lps"] == sq.stats["edit_pair_lps"] == 0
        _same_object(sq, _queries(As, bs, n, now))
    assert sq.scene.calls == ["centers", "bounds", "candidate_pairs", "overlaps"] + [w + "_regions" for w, _ in steps]


def _count_host_decisions(monkeypatch):
    calls = []
    def counted(*a, **k):
        calls.append(1)
        return polytopes_overlap(*a, **k)
    monkeypatch.setattr(gr, "polytopes_overlap", counted)
    import gcs_admm_amd.queries as q
    monkeypatch.setattr(q, "polytopes_overlap", counted)
    return calls


def test_undecided_pairs_are_decided_on_the_host_once(monkeypatch):
    As, bs, n = _regions("benchmark4")
    keys = list(As)
    polys = [(As[k], bs[k]) for k in keys]
    pa, pb = sc.candidate_pairs(*FakeEditScene(polys)._boxes())
    P0 = len(keys) - 3
    old = [t for t in range(len(pa)) if pb[t] < P0][:2]
    new = [t for t in range(len(pa)) if pb[t] >= P0][:2]
    assert len(old) == 2 and len(new) == 2
    undecided = [(_sig(polys[pa[t]]), _sig(polys[pb[t]])) for t in old + new]
    calls = _count_host_decisions(monkeypatch)
    sq = _queries(As, bs, n, keys[:P0], undecided=undecided)
    assert len(calls) == 2 and sq.stats["overlaps_redone_on_host"] == 2
    sq.add_regions({k: As[k] for k in keys[P0:]}, {k: bs[k] for k in keys[P0:]})
    assert len(calls) == 4 and sq.stats["overlaps_redone_on_host"] == 4              # the two new ones alone were solved
    ref = _queries(As, bs, n, keys)                                                  # (decides all four itself)
    assert np.array_equal(sq.edge_tail, ref.edge_tail) and np.array_equal(sq.edge_head, ref.edge_head)
    before = len(calls)
    sq.remove_regions([keys[-1]])
    assert len(calls) == before                                                      # a removal solves nothing
    left = _queries(As, bs, n, keys[:-1], undecided=undecided)
    assert np.array_equal(sq.edge_tail, left.edge_tail) and np.array_equal(sq.edge_head, left.edge_head)
    assert sq.stats["overlaps_redone_on_host"] == left.stats["overlaps_redone_on_host"]


@pytest.mark.parametrize("kind,error,text", [("center", GcsAdmmError, r"centre LP did not converge for regions \['%s'\]"),
                                             ("flat", ValueError, r"regions without interior: \['%s'\]")])
def test_a_failed_centre_or_a_flat_region_raises_and_changes_nothing(kind, error, text):
    As, bs, n = _regions("benchmark2")
    keys = [str(k) for k in As]
    As = {str(k): v for k, v in As.items()}; bs = {str(k): v for k, v in bs.items()}
    sq = _queries(As, bs, n, keys[:-2], bad={_sig((As[keys[-1]], bs[keys[-1]])): kind})
    state = (list(sq.keys), sq.centers.copy(), sq.edge_tail.copy(), sq.edge_head.copy(), dict(sq.stats), len(sq.polys))
    with pytest.raises(error, match=text % keys[-1]):
        sq.add_regions({k: As[k] for k in keys[-2:]}, {k: bs[k] for k in keys[-2:]})
    assert (sq.keys, dict(sq.stats), len(sq.polys)) == (state[0], state[4], state[5])
    assert np.array_equal(sq.centers, state[1]) and np.array_equal(sq.edge_tail, state[2]) and np.array_equal(sq.edge_head, state[3])
    assert len(sq.scene.polys) == len(keys) - 2
    sq.add_regions({keys[-2]: As[keys[-2]]}, {keys[-2]: bs[keys[-2]]})                # the object still works
    _same_object(sq, _queries(As, bs, n, keys[:-1]))


def test_key_errors_come_before_any_scene_call():
    As, bs, n = _regions("benchmark2")
    keys = list(As)
    sq = _queries(As, bs, n, keys[:-1])
    calls = list(sq.scene.calls)
    box = gr.convert_pt_to_polytope(np.zeros(n), 0.1)
    with pytest.raises(ValueError, match="already"):
        sq.add_regions({keys[-1]: As[keys[-1]], keys[0]: As[keys[0]]}, bs)
    for k in ('s', 't'):
        with pytest.raises(ValueError, match="'s' and 't'"):
            sq.add_regions({k: box[0]}, {k: box[1]})
    with pytest.raises(ValueError, match="not in the scene"):
        sq.remove_regions([keys[0], keys[-1]])
    with pytest.raises(ValueError, match="twice"):
        sq.remove_regions([keys[0], keys[0]])
    assert sq.scene.calls == calls and sq.keys == keys[:-1]
