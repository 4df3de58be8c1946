"""The state transfer (csrc/state_transfer_core.h) through its host build, without a device: export then import as the identity, the
table of different graphs, rho and mu_scale, a batch against solo calls, the refusals, and seeded errors in a copy of the header -- all
against ``state_transfer_cases.transfer_reference``, bit for bit, the lanes run forwards and backwards.  The kernels run the same tables
in test_gpu_state_transfer.py.  The front end (``SceneQueries`` ids, ``keep`` / ``seed``) and the claim itself, on the oracle, are in
test_replanning.py."""
import ctypes as C

import numpy as np
import pytest

import hostemu_lib
import state_transfer_cases as X
from gcs_admm_amd import abi
from mutant_build import build_mutants


# ------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("label,s", list(X.round_trip_cases()), ids=[l for l, _ in X.round_trip_cases()])
def test_export_then_import_is_the_identity(label, s):
    for backwards in (False, True):
        snap, state = X.emu_transfer(s, X.Side(s.g, s.ids, s.columns, s.dtype, fill="nan"), backwards=backwards)
        X.same_state(state, s.state, (label, backwards))
        X.same_snapshot(snap, X.export_reference(s), (label, backwards))


def test_a_larger_snapshot_takes_the_members_sizes():
    s = X.side(2, 65)
    snap, state = X.emu_transfer(s, X.Side(s.g, s.ids, fill="nan"), slack=9)
    assert (snap["V"], snap["E"]) == (s.g.num_vertices, s.g.num_edges)
    X.same_snapshot(snap, X.export_reference(s))
    X.same_state(state, s.state)
    assert np.all(snap["edge_key"][s.g.num_edges:] == -5)              # nothing beyond what the member has


# ------------------------------------------------------------------------------------------- different graphs
def _check_pairs(cases, lib=None):
    seen = 0
    for label, src, dst in cases:
        want = X.transfer_reference(src, dst)
        for backwards in (False, True):
            _, state = X.emu_transfer(src, dst, backwards=backwards, lib=lib)
            X.same_state(state, want, (label, backwards))
        seen += 1
    return seen


@pytest.mark.parametrize("dtype,columns", [("f64", ("incidence", "edge")), ("f32", ("edge", "incidence")), ("f64", ("edge", "edge")),
                                           ("f32", ("incidence", "incidence"))])
def test_different_graphs_equal_the_reference(dtype, columns):
    assert _check_pairs(X.pair_cases(dtype=dtype, columns=columns)) >= 2 * len(X.SIZES) + 6


def test_keys_beside_every_source_key():
    assert _check_pairs(X.neighbour_key_cases()) == 5


def test_the_cases_are_what_they_say():
    cases = {label: (src, dst) for label, src, dst in X.pair_cases()}
    assert sorted(src.g.num_edges for label, (src, _) in cases.items() if label.startswith("same-E")) == list(X.SIZES)
    src, dst = cases["disjoint"]
    want = X.transfer_reference(src, dst)
    assert all(not want[k].any() for k in X.STATE)
    src, dst = cases["pruned-E257"]
    assert 0 < dst.g.num_edges < src.g.num_edges and set(dst.ids) < set(src.ids)
    assert X.transfer_reference(src, dst)["zedge"].any()
    src, dst = cases["superset"]
    want = X.transfer_reference(src, dst)["zedge"]
    assert set(src.ids) < set(dst.ids) and want.any() and not want.all(axis=0).all()      # matched and unmatched edges
    src, dst = cases["high-ids"]
    assert src.ids.max() == X.ID_MAX
    low = lambda s: sorted((int(s.ids[u]) << 32 | int(s.ids[w])) & 0xFFFFFFFF for u, w in zip(s.g.edge_tail, s.g.edge_head))
    assert len(set(low(src))) < src.g.num_edges                                           # a 32-bit key would collide
    src, dst = cases["terminal-edges"]
    ends = lambda s: {(int(u), int(w)) for u, w in zip(s.g.edge_tail, s.g.edge_head) if min(u, w) < 2}
    assert ends(src) - ends(dst) and ends(dst) - ends(src)
    for label, src, dst in X.neighbour_key_cases():
        matched = X.transfer_reference(src, dst)["zedge"].any(axis=0)
        assert matched.all() if label == "at" else not matched.any(), label


# ------------------------------------------------------------------------------------------- rho and mu_scale
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rho_and_mu_scale_round_twice_and_touch_mu_alone(dtype):
    T = X.NP_DTYPE[dtype]
    src = X.side(2, 65, dtype=dtype, rho=4.5, mu_scale=1.0 / 3.0, seed=4)
    dst = X.Side(src.g, src.ids, "edge", dtype, fill="nan", rho=1.0)
    snap, state = X.emu_transfer(src, dst)
    assert snap["rho"][0] == 4.5
    want = X.transfer_reference(src, dst)
    X.same_state(state, want)
    # the two roundings, written out: fl_T(mu_scale * mu), then fl_T(that * fl(4.5 / 1))
    first = ((1.0 / 3.0) * src.state["mu"].astype(np.float64)).astype(T)
    second = (first.astype(np.float64) * (np.float64(4.5) / np.float64(1.0))).astype(T)
    E = src.g.num_edges
    assert state["mu"][:, :E].tobytes() == np.ascontiguousarray(second[:, src.tail_col]).tobytes()
    assert state["mu"][:, E:].tobytes() == np.ascontiguousarray(second[:, src.head_col]).tobytes()
    assert not np.array_equal(second, (1.5 * src.state["mu"].astype(np.float64)).astype(T))        # one rounding is another number
    assert state["copy"][:, :E].tobytes() == np.ascontiguousarray(src.state["copy"][:, src.tail_col]).tobytes()
    assert state["zedge"].tobytes() == src.state["zedge"].tobytes() and state["xv"].tobytes() == src.state["xv"].tobytes()


# ------------------------------------------------------------------------------------------- a batch
def test_a_batch_with_a_null_snapshot_equals_the_solo_calls():
    sources = [X.side(2, E, columns=("incidence", "edge")[k % 2], seed=k) for k, E in enumerate((5, 257, 64, 1, 300))]
    drops = [np.arange(s.g.num_vertices) % 4 != 3 for s in sources]
    dests = [X.subgraph_side(s, d, columns=("edge", "incidence")[k % 2], fill="nan") for k, (s, d) in enumerate(zip(sources, drops))]
    for backwards in (False, True):
        src_m = [X.EmuMember(s) for s in sources]
        dst_m = [X.EmuMember(d.with_state(d.state)) for d in dests]
        snaps = [X.snapshot_for(s) for s in sources]
        snaps[2] = None
        rc, text = X.emu_call(src_m, snaps, True, backwards=backwards)
        assert rc == X.OK, text
        rc, text = X.emu_call(dst_m, snaps, False, backwards=backwards, ids=[None if k == 2 else d.ids for k, d in enumerate(dests)])
        assert rc == X.OK, text
        for k, (s, d, m) in enumerate(zip(sources, dests, dst_m)):
            if k == 2:                                                   # not touched
                X.same_state(m.side.state, d.state, k)
                continue
            solo_snap, solo_state = X.emu_transfer(s, d)
            X.same_state(m.side.state, solo_state, k)
            X.same_snapshot(snaps[k].read(), solo_snap, k)
            X.same_state(m.side.state, X.transfer_reference(s, d), k)
        for m in src_m + dst_m:
            m.close()


# ------------------------------------------------------------------------------------------- refusals
def _refusals():
    """(label, text, exporting, member keywords, snapshot edits, ids or None, null state field or None)"""
    s = X.side(2, 20, seed=6)
    V = s.g.num_vertices
    neg = s.ids.copy(); neg[0] = -1
    flat = s.ids.copy(); flat[5] = flat[4]
    down = s.ids.copy(); down[[3, 4]] = down[[4, 3]]
    unsorted = X.Side(X.graph_of(2, 5, [2, 3, 2], [3, 4, 4]), [0, 1, 2, 3, 4])
    twice = X.Side(X.graph_of(2, 5, [2, 2, 3], [3, 3, 4]), [0, 1, 2, 3, 4])
    both = (True, False)
    cases = [("negative id", "vertex ids", both, s, {}, {}, neg, None),
             ("equal ids", "vertex ids", both, s, {}, {}, flat, None),
             ("descending ids", "vertex ids", both, s, {}, {}, down, None),
             ("edge list not ascending", "not strictly ascending", both, unsorted, {}, {}, None, None),
             ("an edge twice", "not strictly ascending", both, twice, {}, {}, None, None),
             ("n differs", "n or state_dtype", both, s, {}, dict(n=3), None, None),
             ("state_dtype differs", "n or state_dtype", both, s, {}, dict(state_dtype=abi.F32), None, None),
             ("snapshot with fewer edges", "smaller", (True,), s, {}, dict(E=19), None, None),
             ("snapshot with fewer vertices", "smaller", (True,), s, {}, dict(V=V - 1), None, None),
             ("ghost columns", "ghost columns", both, s, dict(num_incidences=2 * 20 + 3), {}, None, None),
             ("no reset", "gcsadmm_reset", both, s, dict(reset=False), {}, None, None),
             ("null ids", "null", both, s, {}, {}, "null", None)]
    cases += [(f"null snapshot {f}", "null snapshot array", both, s, {}, {f: None}, None, None) for f in X.SNAPSHOT]
    cases += [(f"null state {f}", "null state pointer", both, s, {}, {}, None, f) for f in X.STATE]
    return cases


def test_refused_calls_return_their_status_and_write_nothing():
    cases = _refusals()
    assert len(cases) >= 23
    for label, text, directions, s, member_kw, snap_edit, ids, null_state in cases:
        for exporting in directions:
            for solo in (True, False):
                m = X.EmuMember(X.Side(s.g, s.ids, s.columns, s.dtype, fill="nan" if not exporting else "random", seed=1), **member_kw)
                before = {k: a.copy() for k, a in m.side.state.items()}
                snap = X.snapshot_for(s)
                if not exporting:                                        # a snapshot an import could read
                    src = X.EmuMember(X.Side(s.g, np.arange(s.g.num_vertices), s.columns, s.dtype))
                    X.emu_call([src], [snap], True, solo=True)              # (refused for the graphs no call takes: the fill stays)
                    src.close()
                filled = {k: a.copy() for k, a in snap.arrays.items()}
                for f, v in snap_edit.items():
                    setattr(snap.c, f, v)
                if null_state:
                    setattr(m.c_state, null_state, None)
                rc, got = X.emu_call([m], [snap], exporting, solo=solo, ids=[None if isinstance(ids, str) else (s.ids if ids is None else ids)])
                assert rc == X.BAD_ARG, (label, exporting, solo)
                assert text in got and got.startswith("" if solo else "member 0: "), (label, got)
                X.same_state(m.side.state, before, label)
                assert all(filled[k].tobytes() == snap.arrays[k].tobytes() for k in X.SNAPSHOT), label
                m.close()
    # a batch: one refused member stops the whole call, also for the members before it; null arrays of pointers
    good, bad = X.side(2, 9, seed=1), X.side(2, 9, seed=2)
    members = [X.EmuMember(good), X.EmuMember(bad)]
    snaps = [X.snapshot_for(good), X.snapshot_for(bad)]
    rc, got = X.emu_call(members, snaps, True, ids=[good.ids, -bad.ids])
    assert rc == X.BAD_ARG and got.startswith("member 1: vertex ids") and np.all(snaps[0].arrays["edge_key"] == -5)
    lib = X.emu()
    handles = (C.c_void_p * 2)(*[m.h for m in members])
    assert lib.ste_transfer(2, handles, (abi.State * 2)(*[m.c_state for m in members]), None, None, 1, 0, 0) == X.BAD_ARG
    assert "null vertex_ids or snapshots" in lib.ste_last_error().decode()
    for m in members:
        m.close()


# ------------------------------------------------------------------------------------------- seeded errors
# (anchor in state_transfer_core.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "search_upper_bound_off_by_one": [("int lo = 0, hi = count - 1;\n    while (lo <= hi) {", "int lo = 0, hi = count - 2;\n    while (lo <= hi) {")],
    "head_column_for_the_tail": [("const size_t to_tail = (size_t)transfer_tail_col(e, edge);", "const size_t to_tail = (size_t)transfer_head_col(e, edge);")],
    "ratio_inverted": [("return rho_snapshot / rho_member;", "return rho_member / rho_snapshot;")],
    "unmatched_edges_left_unwritten": [("const int words = e.c;", "const int words = s >= 0 ? e.c : 0;")],
}
SEEDED = [m for m in MUTANTS if m != "clean"]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    made = build_mutants(tmp_path_factory.mktemp("transfer_mutants"), "state_transfer_core.h", MUTANTS, X.EMU_SRC, flags=[hostemu_lib.INCLUDE])
    return {name: X.declare(lib) for name, lib in made.items()}


def _violations(lib):
    missed = []
    s = X.side(2, 65, seed=8)
    r = X.side(2, 20, rho=4.5, seed=3)
    trips = [("round trip", s, X.Side(s.g, s.ids, "edge", "f64", fill="nan")), ("rho", r, X.Side(r.g, r.ids, fill="nan", rho=1.0))]
    for label, src, dst in trips + [c for c in X.pair_cases() if c[0] in ("pruned-E64", "superset")]:
        try:
            X.same_state(X.emu_transfer(src, dst, lib=lib)[1], X.transfer_reference(src, dst), label)
        except AssertionError:
            missed.append(label)
    return missed


def test_clean_copy_passes(builds):
    assert _violations(builds["clean"]) == []


@pytest.mark.parametrize("mutant", SEEDED)
def test_seeded_errors_are_rejected(builds, mutant):
    assert _violations(builds[mutant]), mutant
