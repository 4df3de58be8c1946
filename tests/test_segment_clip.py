"""The spans of segments in regions and the cover test (csrc/segment_clip_core.h), checked on the host build of the shared core
(tests/hostemu/clip_emu.cpp) against answers that do not come from it: the exact spans of the two relaxed regions of the contract in
``fractions.Fraction`` (cover_cases.exact_span), a Python greedy sweep, closed forms of crafted cases.  The kernels are held to this host
build byte for byte by test_gpu_segment_clip.py.  Also here: seeded errors in the core, ``SceneQueries.path_cover`` and
``queries.rounded_polyline`` with a stand-in scene, the structure of the three entry points, the compiler's resource remarks and a
sanitizer run of a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

import cover_cases as cc
import hostemu_lib
import locate_cases as lc
from gcs_admm_amd import build, queries
from gcs_admm_amd.native_build import build_library
from gcs_admm_amd.queries import SceneQueries
from mutant_build import build_mutants
from test_query_graph import AssemblyScene


# ------------------------------------------------------------------------------------------- the checks
def check_list(res, num, P):
    """the list's own consistency (locate_cases.dense) and that of the spans and the chains; returns the class matrix [Q, P] and the
    list position of every pair [Q, P] (-1: not listed)"""
    hit_ptr, region, cls, t_in, t_out, status, reach, chain_ptr, chain = res
    M = lc.dense(res[:3], num, P)
    assert t_in.dtype == t_out.dtype == reach.dtype == np.float64 and status.dtype == chain.dtype == np.int32 and chain_ptr.dtype == np.int64
    assert t_in.shape == t_out.shape == region.shape and status.shape == reach.shape == (num,) and chain_ptr.shape == (num + 1,)
    assert np.all((0.0 <= t_in) & (t_in <= t_out) & (t_out <= 1.0))
    assert np.array_equal(cls == cc.WHOLE, (t_in == 0.0) & (t_out == 1.0))
    assert chain_ptr[0] == 0 and chain_ptr[-1] == len(chain) and np.all(np.diff(chain_ptr) >= 0) and np.all(np.diff(chain_ptr) <= np.diff(hit_ptr))
    at = np.full((num, P), -1, np.int64)
    at[np.repeat(np.arange(num, dtype=np.int64), np.diff(hit_ptr)), region] = np.arange(len(region))
    return M, at


def check_sandwich(res, polys, start, end, tol=cc.TOL):
    """every listed span contains the exact inner span and lies in the exact outer one; every pair with a non-empty inner span is
    listed, none with an empty outer span is.  Returns (pairs in between, hits)"""
    num, P = len(start), len(polys)
    M, at = check_list(res, num, P)
    exact = cc.exact_spans(polys, start, end, tol)
    between = 0
    for q in range(num):
        for r in range(P):
            inner, outer = exact.get((q, r), (None, None))
            t = at[q, r]
            if inner is not None:
                assert t >= 0, ("a pair with a non-empty inner span is not listed", q, r)
            if outer is None:
                assert t < 0, ("a pair with an empty outer span is listed", q, r)
            between += inner is None and outer is not None
            if t >= 0:
                lo, hi = cc.F(float(res[3][t])), cc.F(float(res[4][t]))
                assert outer[0] <= lo and hi <= outer[1], ("outside the outer span", q, r, float(lo - outer[0]), float(outer[1] - hi))
                if inner is not None:
                    assert lo <= inner[0] and inner[1] <= hi, ("does not contain the inner span", q, r, float(inner[0] - lo), float(hi - inner[1]))
    return between, int((M != 0).sum())


def check_own_sweep(res):
    """status, reach and chain are what a Python sweep makes of the call's own spans, exactly"""
    status, reach, chain_ptr, chain = cc.own_sweep(res)
    for got, want, what in zip(res[5:], (status, reach, chain_ptr, chain), cc.FIELDS[5:]):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), what
    assert np.all(res[6][res[5] == cc.COVERED] == 1.0) and np.all(res[6][res[5] == cc.GAP] < 1.0)


def check_crafted(res, names, polys, start, end, expect):
    check_list(res, len(start), len(polys))
    hit_ptr, region, _, _, _, status, reach, chain_ptr, chain = res
    for q, (st, r, ch) in expect.items():
        got = [names[region[c]] for c in chain[chain_ptr[q]:chain_ptr[q + 1]]]
        assert status[q] == st and got == ch, (q, int(status[q]), got)
        assert reach[q] == r if r in (0.0, 1.0) else abs(reach[q] - r) < 1e-11, (q, float(reach[q]), r)
    check_own_sweep(res)


def exact_status(polys, start, end, which):
    """the status per segment of the greedy sweep over the exact inner (0) or outer (1) spans"""
    exact = cc.exact_spans(polys, start, end)
    out = []
    for q in range(len(start)):
        spans = [exact[(q, r)][which] for r in range(len(polys)) if (q, r) in exact and exact[(q, r)][which] is not None]
        out.append(cc.sweep(spans)[0])
    return np.array(out, np.int32)


# ------------------------------------------------------------------------------------------- spans on the locate families
def test_the_host_build_has_the_kernels_chunk():
    assert cc.emu().clip_emu_chunk() == lc.CHUNK and max(cc.SIZES) > 2 * lc.CHUNK


@pytest.mark.parametrize("n", lc.DIMS)
@pytest.mark.parametrize("kind,offset", lc.FAMILIES)
def test_spans_obey_the_sandwich_and_the_list_is_complete(kind, offset, n):
    hits = 0
    for P in cc.SIZES:
        polys, start, end, res = cc.family(kind, n, P, offset)
        between, h = check_sandwich(res, polys, start, end)
        print(kind, offset, n, P, "hits", h, "pairs in between", between)
        assert between <= 0.01 * cc.Q * P
        hits += h
        check_own_sweep(res)
        # the whole call is a plain double loop over single pairs, byte for byte
        for got, want, what in zip(res[:5], cc.double_loop(polys, start, end), cc.FIELDS):
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (P, what)
    assert hits >= 12


def test_one_segment_is_the_first_of_twelve():
    for P in cc.SIZES:
        polys, start, end, res = cc.family("polytopes", 3, P, 300.0)
        one = cc.family("polytopes", 3, P, 300.0, 1)[3]
        k, c = res[0][1], res[7][1]
        for a, b in zip(one, (res[0][:2], res[1][:k], res[2][:k], res[3][:k], res[4][:k], res[5][:1], res[6][:1], res[7][:2], res[8][:c])):
            assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------- cover and chain
@pytest.mark.parametrize("rotate", [None, 7])
def test_cover_of_a_lattice_with_a_hole(rotate):
    """status, reach and chain equal the Python sweep over the call's own spans; independently the status equals the sweep over the
    exact inner spans and over the exact outer spans, which agree on these inputs"""
    covered = gaps = longest = 0
    for n, offset in cc.LATTICES:
        polys, start, end, res = cc.lattice_case(n, offset, rotate)
        check_sandwich(res, polys, start, end)
        check_own_sweep(res)
        inner, outer = exact_status(polys, start, end, 0), exact_status(polys, start, end, 1)
        assert np.array_equal(inner, outer), "the inputs do not separate the two relaxations"
        assert np.array_equal(res[5], inner)
        covered += int((res[5] == cc.COVERED).sum()); gaps += int((res[5] == cc.GAP).sum()); longest = max(longest, int(np.diff(res[7]).max()))
    print("rotated" if rotate else "axis-aligned", "covered", covered, "gap", gaps, "longest chain", longest)
    assert covered >= 40 and gaps >= 20 and longest >= 4


# ------------------------------------------------------------------------------------------- crafted cases
def test_crafted_cases():
    names, polys, start, end, expect = cc.crafted()
    res = cc.emu_clip(polys, start, end)
    check_crafted(res, names, polys, start, end, expect)
    check_sandwich(res, polys, start, end)
    M, at = check_list(res, len(start), len(polys))
    assert M[2, names.index("up")] == M[2, names.index("down")] == cc.WHOLE          # along the shared face: WHOLE in both
    assert M[3, names.index("a")] == cc.WHOLE and M[3].astype(bool).sum() == 1        # a point: [0, 1] or nothing
    assert not M[4].any() and M[5, names.index("a")] == cc.PART
    t1, t2 = at[6, names.index("tie1")], at[6, names.index("tie2")]
    assert res[4][t1] == res[4][t2] and res[3][t1] == res[3][t2] == 0.0               # a true tie, decided by the index


def test_rows_of_zeros_and_regions_without_rows():
    names, polys, start, end = cc.zero_row_case()
    res = cc.emu_clip(polys, start, end)
    M, _ = check_list(res, 2, len(polys))
    assert M.tolist() == [[cc.WHOLE, cc.WHOLE, 0, cc.WHOLE], [0, cc.WHOLE, 0, cc.WHOLE]]
    assert res[5].tolist() == [cc.COVERED, cc.COVERED] and [names[res[1][c]] for c in res[8]] == ["unit", "zero_whole"]
    check_own_sweep(res)


def test_a_chain_longer_than_a_stride():
    polys, start, end = cc.collinear(130)
    res = cc.emu_clip(polys, start, end)
    assert res[0].tolist() == [0, 130] and res[5].tolist() == [cc.COVERED]
    assert len(res[8]) > 64 and np.all(np.diff(res[1][res[8]]) >= 1)
    check_own_sweep(res)
    check_sandwich(res, polys, start, end)


def test_empty_calls():
    res = cc.emu_clip(cc.crafted()[1], np.zeros((0, 2)), np.zeros((0, 2)))
    assert res[0].tolist() == [0] and res[7].tolist() == [0] and all(len(a) == 0 for a in res[1:7] + res[8:])
    res = cc.emu_clip([], np.zeros((2, 2)), np.ones((2, 2)), n=2)
    assert res[0].tolist() == [0, 0, 0] and res[5].tolist() == [cc.GAP, cc.GAP] and res[6].tolist() == [0.0, 0.0] and res[7].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------- seeded errors
# (anchor in segment_clip_core.h, replacement): each anchor must occur exactly once
MUTANTS = {
    "clean": [],
    "no_allowance": [("const double m = fma(tol, s, 0x1p-40 * mag);", "const double m = tol * s;")],
    "strict_start": [("if (in <= cur && cur < out", "if (in < cur && cur < out")],
    "reversed_tie": [("(a_out == b_out && a_pos < b_pos)", "(a_out == b_out && a_pos > b_pos)")],
}


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    libs = build_mutants(tmp_path_factory.mktemp("clip_mutants"), "segment_clip_core.h", MUTANTS, os.path.join(hostemu_lib.HOSTEMU, "clip_emu.cpp"),
                         flags=["-ffp-contract=off"])
    return {name: cc.bind(lib) for name, lib in libs.items()}


def failures(lib):
    """the checks a build misses: the sandwich on two family members, the crafted cases, a lattice against the exact sweeps"""
    out = []

    def run(name, check):
        try:
            check()
        except AssertionError:
            out.append(name)

    def sandwich():
        for kind, n, P, offset in (("polytopes", 2, 65, 0.0), ("scaled", 3, 65, 300.0)):
            polys = lc.regions(kind, n, P, offset)
            start, end = cc.segments(kind, n, P, offset)
            check_sandwich(cc.emu_clip(polys, start, end, lib=lib), polys, start, end)

    def crafted():
        names, polys, start, end, expect = cc.crafted()
        check_crafted(cc.emu_clip(polys, start, end, lib=lib), names, polys, start, end, expect)

    def lattice():
        polys, start, end = cc.lattice(2)
        res = cc.emu_clip(polys, start, end, lib=lib)
        check_own_sweep(res)
        assert np.array_equal(res[5], exact_status(polys, start, end, 0))

    run("sandwich", sandwich); run("crafted", crafted); run("lattice", lattice)
    return out


def test_the_clean_copy_passes(builds):
    assert failures(builds["clean"]) == []


@pytest.mark.parametrize("mutant,seen_by", [("no_allowance", "sandwich"), ("strict_start", "crafted"), ("reversed_tie", "crafted")])
def test_seeded_errors_are_rejected(builds, mutant, seen_by):
    found = failures(builds[mutant])
    print(mutant, found)
    assert seen_by in found


# ------------------------------------------------------------------------------------------- SceneQueries on a stand-in scene
class ClipScene(AssemblyScene):
    """AssemblyScene with the one call the cover test adds, from the host build"""

    def __init__(self, polys, pairs):
        AssemblyScene.__init__(self, polys, pairs)
        self.clip_calls = []

    def clip_segments(self, start, end, tol=1e-9):
        p, q = (np.ascontiguousarray(x, float).reshape(-1, self.n) for x in (start, end))
        self.clip_calls.append((p.copy(), q.copy(), tol))
        return cc.emu_clip(self.polys, p, q, tol, n=self.n)


def queries_on(name):
    As, bs, n, pairs = lc.region_sets(name)
    scene = ClipScene([(np.asarray(As[k], float), np.asarray(bs[k], float).ravel()) for k in As], pairs)
    return scene, SceneQueries(As, bs, n, scene=scene, pair_lp=lc.PairLP())


def test_path_cover_on_four_boxes():
    """boxes 0: [0, 1]^2, 1: [0.9, 2] x [0, 1], 2: [1.9, 3] x [0, 1], 3: [8, 9]^2; edges 0-1 and 1-2"""
    scene, sq = queries_on("four_boxes")
    with sq:
        through = np.array([[0.2, 0.5], [1.5, 0.5], [2.8, 0.5]])
        away = np.array([[0.5, 0.5], [0.75, 0.75], [8.5, 8.5]])
        got = sq.path_cover([through, away, through[::-1]])
        assert len(scene.clip_calls) == 1 and len(scene.clip_calls[0][0]) == 6          # all segments of all paths in one call
        a, b, c = got
        # region 1 ends the first segment and begins the second: merged across the polyline's vertex
        assert a["covered"] and a["gap"] is None and a["corridor"] == [0, 1, 2] and a["adjacent"]
        assert len(a["breaks"]) == 2 and np.allclose(a["breaks"], [[1.0, 0.5], [2.0, 0.5]], rtol=0, atol=2e-9)
        assert c["covered"] and c["corridor"] == [2, 1, 0] and np.allclose(c["breaks"], [[1.9, 0.5], [0.9, 0.5]], rtol=0, atol=2e-9)
        # the second path leaves box 0 through its corner (1, 1) in its second segment, 0.25 / 7.75 of the way
        assert not b["covered"] and b["corridor"] == [0] and b["breaks"] == [] and b["adjacent"]
        assert b["gap"]["segment"] == 1 and abs(b["gap"]["t"] - 0.25 / 7.75) < 1e-9 and np.allclose(b["gap"]["point"], [1.0, 1.0], rtol=0, atol=2e-9)
        assert np.array_equal(b["gap"]["point"], away[1] + b["gap"]["t"] * (away[2] - away[1]))
        # an inflation of half a unit: box 2 holds the point where box 0 ends and reaches further than box 1; 0-2 is no edge of the graph
        wide = sq.path_cover([through[[0, 2]]], tol=0.5)[0]
        assert wide["covered"] and wide["corridor"] == [0, 2] and not wide["adjacent"]
        assert sq.path_cover([]) == []
        with pytest.raises(ValueError, match="at least two points"):
            sq.path_cover([through[:1]])
    with pytest.raises(RuntimeError, match="closed"):
        sq.path_cover([through])


def test_rounded_polyline_walks_the_rounded_path():
    scene, sq = queries_on("four_boxes")
    with sq:
        g = sq.graphs(np.array([[0.5, 0.5]]), np.array([[2.5, 0.5]]))[0]
    q = np.array([[0.5, 0.5], [0.5, 0.5], [0.95, 0.4], [1.95, 0.6], [2.5, 0.5], [2.5, 0.5]])
    path = ['s', 0, 1, 2, 't']
    xs = {v: np.zeros(4) for v in g.keys}
    xs.update({v: np.concatenate([q[j], q[j + 1]]) for j, v in enumerate(path)})
    record = dict(graph=g, x_v_rounded=xs, y_v_rounded={v: int(v in path) for v in g.keys})
    got = queries.rounded_polyline(record)
    assert got.tobytes() == q[1:5].tobytes()                                            # the repeated end points dropped
    scene, sq = queries_on("four_boxes")
    with sq:
        cover = sq.path_cover([got])[0]
    assert cover["covered"] and cover["corridor"] == [0, 1, 2] and cover["adjacent"]
    with pytest.raises(ValueError, match="no rounded path"):
        queries.rounded_polyline(dict(graph=g, x_v_rounded=None, y_v_rounded=None))
    broken = dict(record, y_v_rounded={v: int(v in ('s', 0, 't')) for v in g.keys})      # 0 has no successor that continues it
    with pytest.raises(ValueError, match="ends at 0"):
        queries.rounded_polyline(broken)


# ------------------------------------------------------------------------------------------- the entry points, the product's kernels
def _body(src, name):
    at = src.index(f"\nint {name}(")
    start = src.index("{", src.index(")", at))
    depth, i = 1, start + 1
    while depth:
        depth += (src[i] == "{") - (src[i] == "}")
        i += 1
    return src[start:i]


def test_entry_points_refuse_before_they_touch_the_list():
    """the three entry points are one ``scene_entry`` each; every refusal of clip_segments stands in front of ``stage_start`` (so a
    refused call leaves the earlier list), the count of hits is checked before the list is allocated, the call takes the row of
    locate_points, every call that makes a list says which kind it leaves, and each read asks for its kind before it copies.
    (test_gpu_segment_clip.py runs them.)"""
    src = open(os.path.join(build.CSRC, "polytope_lp.hip")).read()
    body = _body(src, "gcsadmm_scene_clip_segments")
    assert re.match(r"\{\s*return scene_entry\(s, \[&\]\(\) -> int \{", body)
    start = body.index("stage_start(s->have, CALL_LOCATE_POINTS);")
    for text in ("negative number of segments or null end points", "tol must be finite and non-negative", "segment with a NaN or an inf coordinate"):
        assert 0 < body.index(text) < start, text
    assert body.count("GCSADMM_ERR_BAD_ARG") == 3 and body.index("GCSADMM_ERR_BAD_ARG", start - 200) < start
    assert start < body.index("more than 2^31 - 1 hits") < body.index("h.region.reserve(")
    assert body.index("h.clipped = true;") < body.index("stage_finish(s->have, CALL_LOCATE_POINTS);")
    assert "h.projected = false;" in body
    for name in ("gcsadmm_scene_read_spans", "gcsadmm_scene_read_cover"):
        read = _body(src, name)
        assert re.match(r"\{\s*return scene_entry\(s, \[&\]\(\) -> int \{\s*NEED\(s, CALL_READ_HITS\);", read), name
        assert read.index("if (!h.clipped)") < read.index("to_host("), name
    assert src.count("s->hits.clipped = false;") == 2 and src.count(" h.clipped = false;") == 1      # the two locate calls, project_points
    assert "if (!h.projected)" in _body(src, "gcsadmm_scene_read_projections")
    header = open(os.path.join(build.ROOT, "include", "gcsadmm.h")).read()
    for name in ("gcsadmm_scene_clip_segments", "gcsadmm_scene_read_spans", "gcsadmm_scene_read_cover"):
        assert f"int {name}(gcsadmm_scene s," in header


def test_both_kernels_keep_their_working_set_in_registers():
    res = {k: v for k, v in build.kernel_resources().items() if "segment_clip_kernel" in k or "segment_chain_kernel" in k}
    assert len([k for k in res if "segment_clip_kernel" in k]) == 16 and len(res) == 17, sorted(res)      # N = 1 .. 8 in two passes; the chain
    for k, v in res.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (k, v)


def test_the_core_runs_clean_under_the_sanitizers():
    """a stand-alone program (its own main) on crafted scenes, compiled with -fsanitize=address,undefined and run here"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    exe = build_library(os.path.join(build.ROOT, "build", "clip_sanitize"), hostemu_lib.sources([("clip_sanitize.cpp", [])]),
                        flags=hostemu_lib.FLAGS + ["-ffp-contract=off"] + san, link_flags=san)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok" and p.stderr == "", (p.returncode, p.stdout, p.stderr)
