"""The projection of points onto regions (csrc/point_project_core.h: the candidate list, the dual active-set solve, the statuses), checked
on the host build of the shared core (tests/hostemu/project_emu.cpp) against answers that do not come from it: a least-distance solve by
``scipy.optimize.nnls`` polished in longdouble (project_cases.reference), a duality certificate the test computes itself, and closed forms
(boxes, rotated cubes).  The kernels are held to this host build byte for byte by test_gpu_point_project.py.  Also here: ``SceneQueries``
with a stand-in scene (``nearest_regions``, ``outside="snap"``), the structure of the two entry points, the compiler's resource remarks and a
stand-alone program under the sanitizers.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import hostemu_lib
import locate_cases as lc
import project_cases as pc
import rotated_cases
from gcs_admm_amd import build
from gcs_admm_amd.native_build import build_library
from gcs_admm_amd.queries import SceneQueries
from test_query_graph import AssemblyScene, assert_same_graphs

L = np.longdouble
WORST = {"feasibility": 0.0, "gap": 0.0, "iterations": 0}      # printed by the last test: what profiles/project/README.md records


def check_sound(polys, pts, res, skip=()):
    """feasibility and optimality of every solved hit (but the list entries ``skip``); returns the number of hits checked"""
    point_of = np.repeat(np.arange(len(pts)), np.diff(res[0]))
    for t in np.nonzero(res[5] >= 0)[0]:
        if t in skip:
            continue
        A, b = polys[res[1][t]]
        p, x = pts[point_of[t]], res[4][t]
        feas = pc.feasibility(A, b, x)
        assert feas <= pc.ALLOW, ("feasibility", t, float(feas))
        gap, scale = pc.certificate(A, b, p, x)
        assert gap <= L(1e-9) * scale, ("certificate", t, float(gap), float(scale))
        d = np.sqrt(((x.astype(L) - p.astype(L)) ** 2).sum())
        assert abs(L(res[3][t]) - d) <= L(4 * np.finfo(float).eps) * d, ("distance", t)
        WORST["feasibility"] = max(WORST["feasibility"], float(feas / pc.ALLOW))
        WORST["gap"] = max(WORST["gap"], float(gap / scale))
    WORST["iterations"] = max(WORST["iterations"], int(res[6].max()) if len(res[6]) else 0)
    return int((res[5] >= 0).sum())


@pytest.mark.parametrize("n", lc.DIMS)
@pytest.mark.parametrize("kind,offset", lc.FAMILIES)
def test_families_complete_sound_and_in_list_order(kind, offset, n):
    assert pc.emu().project_emu_chunk() == lc.CHUNK and max(pc.SIZES) > 2 * lc.CHUNK
    for P in pc.SIZES:
        polys, pts, rad, res = pc.family(kind, n, P, offset)
        M, at = pc.dense(res, len(pts), P)
        X, D, low = pc.reference_call(polys, pts, rad)          # (D = +inf: beyond the radius and not one of the two nearest)
        solved = np.isfinite(D)
        # the conditions on the inputs: no distance at a radius, no two nearest regions at one distance
        finite = solved & np.isfinite(rad)[:, None]
        Df, rf = np.where(finite, D, 0), np.where(finite, rad[:, None], 1)
        assert np.all((np.abs(Df - rf) > L(1e-9) * np.maximum(Df, rf)) | (D == 0)), "a reference distance lies at its point's radius"
        if P > 1:
            two = np.sort(D, axis=1)[:, :2]
            assert np.all(np.isfinite(two)) and np.all((two[:, 1] - two[:, 0] > L(1e-9) * two[:, 1]) | (two[:, 1] == 0)), "two nearest regions at one distance"
        # completeness: every pair within the radius is listed and solved with status 0; nothing failed
        assert not np.any(res[5] == pc.FAILED), int((res[5] == pc.FAILED).sum())
        within = D <= rad[:, None]                               # (an infinite radius: every pair)
        assert np.all(at[within] >= 0)
        assert np.all(res[5][at[within]] == pc.SOLVED)
        listed = at >= 0
        assert np.all(res[5][at[listed & ~within]] == pc.BEYOND)
        assert np.all((M == pc.INSIDE) == (low == 0)) and np.all(D[low == 0] == 0)
        # soundness
        assert check_sound(polys, pts, res) == len(res[1])
        both = listed & solved
        assert np.allclose(res[3][at[both]], D[both].astype(float), rtol=1e-9, atol=1e-9 * 2.0 ** -20 * (np.abs(pts).max() + 1))
        inside = res[2] == pc.INSIDE
        point_of = np.repeat(np.arange(len(pts)), np.diff(res[0]))
        assert np.all(res[6][inside] == 0) and np.all(res[3][inside] == 0) and res[4][inside].tobytes() == pts[point_of[inside]].tobytes()
        # the list of the whole call is the list of a plain double loop over the classification and the solve of single pairs
        if P <= 65 or n == 3:
            for got, want, f in zip(res, pc.double_loop(polys, pts, rad), pc.FIELDS):
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (P, f)
        if kind == "boxes":
            for t in range(len(res[1])):
                A, b = polys[res[1][t]]
                lo, hi = -b[n:2 * n] / 1.0, b[:n]
                p = pts[point_of[t]]
                want = np.clip(p, lo, hi)
                same = want == p
                assert np.all(res[4][t][same] == p[same]), "a coordinate that is not clipped moved"
                assert np.all(np.abs(res[4][t] - want) <= 4 * np.spacing(np.abs(want))), (t, res[4][t], want)


@pytest.mark.parametrize("n", [3, 5, 8])
def test_rotated_cubes_match_the_closed_form(n):
    """the cube |R x|_inf <= 1 for an orthogonal R: the projection is R' clip(R p)"""
    R = rotated_cases.rotation(n, 100 + n)
    assert np.allclose(R @ R.T, np.eye(n), atol=1e-14)
    polys = [(np.vstack([R, -R]), np.ones(2 * n))]
    rng = np.random.default_rng(n)
    pts = np.vstack([rng.normal(size=(10, n)) * 2.0, R.T @ np.full(n, 3.0), R.T @ (np.arange(n) % 2 * 2.5), np.zeros(n)])
    res = pc.emu_project(polys, pts)
    assert res[0].tolist() == list(range(len(pts) + 1)) and np.all(res[5] == pc.SOLVED)
    check_sound(polys, pts, res)
    Rl = R.astype(L)
    for q, p in enumerate(pts):
        want = Rl.T @ np.clip(Rl @ p.astype(L), -1, 1)
        d2 = ((want - p) ** 2).sum()
        scale = max(d2, pc.ALLOW * (np.abs(p).max() + 1) ** 2)
        x = res[4][q].astype(L)
        assert abs(((x - p) ** 2).sum() - d2) / 2 <= L(1e-9) * scale
        assert ((x - want) ** 2).sum() <= 2 * L(1e-9) * scale          # (1/2 |x - x*|^2 <= f(x) - f(x*) on the region)
    assert res[2][-1] == pc.INSIDE and res[6][-1] == 0


def check_crafted(res, names, polys, pts, rad, expect):
    """the expectations of the crafted table on the seven arrays of a call (the device test runs it too)"""
    M, at = pc.dense(res, len(pts), len(polys))
    for (q, name), e in expect.items():
        r = names.index(name)
        if e is None:
            assert M[q, r] == pc.OUT, (q, name)
            continue
        cls, status, x, d, its = e
        t = at[q, r]
        assert t >= 0 and (M[q, r], res[5][t]) == (cls, status), (q, name, int(M[q, r]), int(res[5][t]))
        assert np.allclose(res[4][t], x, rtol=0, atol=1e-15) and abs(res[3][t] - d) <= 1e-15 * max(d, 1e-5), (q, name, res[4][t], res[3][t])
        assert its is None or res[6][t] == its, (q, name, int(res[6][t]))
    for q in (0, 1, 5):      # INSIDE: the point itself, bit for bit
        t = at[q, names.index("unit")]
        assert res[4][t].tobytes() == pts[q].tobytes() and res[3][t] == 0.0
    # two regions at one distance: both are listed with the same d; the lower index comes first
    l, r = at[5, names.index("left")], at[5, names.index("right")]
    assert res[3][l] == res[3][r] == 2.0 and l < r


def test_crafted_cases():
    names, polys, pts, rad, expect = pc.crafted()
    res = pc.emu_project(polys, pts, rad)
    check_crafted(res, names, polys, pts, rad, expect)
    # (the apex of the wedge is the origin and its rows have b = 0: the allowance 2^-40 (sum |a_ik x_k| + |b_i|) is 2^-40 of the rounding
    # noise of x itself there, a test of the noise's sign; check_crafted holds that x to 1e-15 of the apex instead)
    check_sound(polys, pts, res, skip=[pc.dense(res, len(pts), len(polys))[1][4, names.index("wedge")]])
    for got, want, f in zip(res, pc.double_loop(polys, pts, rad), pc.FIELDS):
        assert got.tobytes() == want.tobytes(), f


def test_beyond_the_radius_and_iteration_limits():
    polys, pts, rad, d = pc.beyond_case()
    res = pc.emu_project(polys, pts, rad)
    assert res[1].tolist() == [0] and res[5].tolist() == [pc.BEYOND] and abs(res[3][0] - d) < 1e-15 and np.allclose(res[4][0], [1.0, 1.0], rtol=0, atol=1e-15)
    assert pc.emu_project(polys, pts, [0.4])[1].tolist() == []            # the rows alone say so: not listed
    assert pc.emu_project(polys, pts, [0.8])[5].tolist() == [pc.SOLVED]
    # max_iter = 0: every candidate but the INSIDE ones fails, with the point itself as its iterate; max_iter = 1: one step is enough
    # for a point beyond one facet, not beyond a vertex
    names, polys, pts, rad, expect = pc.crafted()
    none, one, full = (pc.emu_project(polys, pts, rad, max_iter=k) for k in (0, 1, pc.MAX_ITER))
    for a, b in zip(none[:3], full[:3]):
        assert a.tobytes() == b.tobytes()                                  # the list does not depend on the limit
    inside = full[2] == pc.INSIDE
    assert np.all(none[5][inside] == pc.SOLVED) and np.all(none[5][~inside] == pc.FAILED) and np.all(none[6] == 0)
    assert np.all(one[5][full[6] <= 1] == full[5][full[6] <= 1]) and np.all(one[5][full[6] > 1] == pc.FAILED) and np.all(one[6] <= 1)
    assert np.any(full[6] > 1) and np.any(full[6] == 1)
    assert one[4][full[6] <= 1].tobytes() == full[4][full[6] <= 1].tobytes()


def test_empty_calls():
    polys = lc.regions("polytopes", 2, 5)
    res = pc.emu_project(polys, np.zeros((0, 2)))
    assert res[0].tolist() == [0] and all(len(a) == 0 for a in res[1:])
    res = pc.emu_project([], np.zeros((2, 2)), n=2)
    assert res[0].tolist() == [0, 0, 0] and all(len(a) == 0 for a in res[1:])


# ------------------------------------------------------------------------------------------- SceneQueries on a stand-in scene
class ProjectScene(AssemblyScene):
    """AssemblyScene with the one call the projections add, from the host build; ``fail``: list entries handed out with status -1 and
    a useless iterate, as a solve that hit its iteration limit leaves them"""

    def __init__(self, polys, pairs, fail=()):
        AssemblyScene.__init__(self, polys, pairs)
        self.project_calls, self.fail = [], fail

    def project(self, points, radius=None, max_iter=100):
        pts = np.ascontiguousarray(points, float).reshape(-1, self.n)
        self.project_calls.append((pts.copy(), None if radius is None else np.array(radius, float)))
        res = [np.array(a) for a in pc.emu_project(self.polys, pts, radius, max_iter, n=self.n)]
        for t in self.fail:
            res[5][t] = -1; res[3][t] = np.nan; res[4][t] = np.nan
        return tuple(res)


def queries_on(name, fail=()):
    As, bs, n, pairs = lc.region_sets(name)
    scene = ProjectScene([(np.asarray(As[k], float), np.asarray(bs[k], float).ravel()) for k in As], pairs, fail)
    return scene, SceneQueries(As, bs, n, scene=scene, pair_lp=lc.PairLP())


OUTSIDE_POINTS = np.array([[-0.05, 0.5],        # 0.05 left of box 0
                           [3.2, 1.3],          # beyond the corner (3, 1) of box 2
                           [1.5, 0.5],          # inside box 1
                           [0.95, -0.1],        # below boxes 0 and 1 where they overlap: equally far from both
                           [6.0, 6.0]])         # nearer to box 3


def test_nearest_regions_agree_with_the_restatement():
    scene, sq = queries_on("four_boxes")
    with sq:
        got = sq.nearest_regions(OUTSIDE_POINTS)
        assert len(scene.project_calls) == 1 and sq.last["redone_on_host"] == 0
        # the default radius: the distance to the nearest centre
        want_rad = np.array([np.sqrt(((sq.centers - p) ** 2).sum(axis=1)).min() for p in OUTSIDE_POINTS])
        assert np.array_equal(scene.project_calls[0][1], want_rad)
        X, D, _ = pc.reference_call(sq.polys, OUTSIDE_POINTS)
        for q, (r, d, x) in enumerate(got):
            assert r == int(np.argmin(D[q])) and abs(d - float(D[q, r])) <= 1e-15 and np.allclose(x, X[q, r].astype(float), rtol=0, atol=1e-15)
        assert [g[0] for g in got] == [0, 2, 1, 0, 3] and got[2][1] == 0.0 and got[2][2].tobytes() == OUTSIDE_POINTS[2].tobytes()
        # an explicit radius, one for all or one per point; a point with nothing within it
        got = sq.nearest_regions(OUTSIDE_POINTS, 0.06)
        assert [g[0] for g in got] == [0, -1, 1, -1, -1] and got[1][1] == np.inf and got[1][2] is None
        got = sq.nearest_regions(OUTSIDE_POINTS[:2], [0.01, 1.0])
        assert [g[0] for g in got] == [-1, 2]


def test_a_failed_device_solve_is_redone_on_the_host_and_counted():
    scene, sq = queries_on("four_boxes", fail=(0, 1))      # the entries of point 0: boxes 0 and 1 under the default radius
    with sq:
        got = sq.nearest_regions(OUTSIDE_POINTS[:2])
        assert sq.last["redone_on_host"] == 2
        assert got[0][0] == 0 and abs(got[0][1] - 0.05) < 1e-8 and np.allclose(got[0][2], [0.0, 0.5], atol=1e-8)
        assert got[1][0] == 2 and abs(got[1][1] - np.hypot(0.2, 0.3)) < 1e-8


@pytest.mark.parametrize("assemble", ["host", "device"])
def test_graphs_snap_equals_graphs_with_the_projected_point(assemble):
    scene, sq = queries_on("four_boxes")
    starts = np.array([[-0.05, 0.5], [0.5, 0.5], [3.2, 1.3]]); goals = np.array([[2.5, 0.5], [2.5, 1.05], [0.2, 0.2]])
    with sq:
        with pytest.raises(ValueError, match=r"^query 0: the start lies in no region$"):          # the default: today's text
            sq.graphs(starts, goals, assemble=assemble)
        keep = starts.copy()
        got = sq.graphs(starts, goals, assemble=assemble, outside="snap")
        assert starts.tobytes() == keep.tobytes()                         # the caller's arrays are not written
        assert len(scene.project_calls) == 1 and len(scene.project_calls[0][0]) == 3          # one project call: the three points outside
        snapped = sq.snapped
        assert [(r["start"] is not None, r["goal"] is not None) for r in snapped] == [(True, False), (False, True), (True, False)]
        rec = snapped[2]["start"]
        assert rec["original"].tolist() == [3.2, 1.3] and rec["point"].tolist() == [3.0, 1.0] and rec["region"] == 2
        assert abs(rec["distance"] - np.hypot(0.2, 0.3)) < 1e-15
        s2, g2 = starts.copy(), goals.copy()
        s2[0], s2[2], g2[1] = (0.0, 0.5), (3.0, 1.0), (2.5, 1.0)
        assert_same_graphs(got, sq.graphs(s2, g2, assemble=assemble))
        assert got[0].interior[0].tolist() == [0.0, 0.5] and got[1].interior[1].tolist() == [2.5, 1.0]
        # a query with nothing outside is what it was, and asks for no projection
        assert_same_graphs(sq.graphs(s2, g2, assemble=assemble, outside="snap"), got)
        assert len(scene.project_calls) == 1 and all(r == dict(start=None, goal=None) for r in sq.snapped)


def test_snap_radius_boxes_and_refusals():
    scene, sq = queries_on("four_boxes")
    starts = np.array([[-0.05, 0.5]]); goals = np.array([[2.5, 0.5]])
    with sq:
        with pytest.raises(ValueError, match=r"query 0: the start lies in no region, and no region is within 0.01 of it"):
            sq.graphs(starts, goals, outside="snap", snap_radius=0.01)
        assert len(sq.graphs(starts, goals, outside="snap", snap_radius=0.06)) == 1
        with pytest.raises(ValueError, match="outside must be 'raise' or 'snap'"):
            sq.graphs(starts, goals, outside="project")
        # box terminals are untouched: a box that meets no region raises as before, whatever `outside` says
        box = (np.array([[4.0, 4.0]]), np.array([[5.0, 5.0]]))
        scene.locate_boxes = lambda lo, hi, tol=lc.TOL: __import__("locate_box_cases").emu_locate_boxes(scene.polys, lo, hi, tol, n=scene.n)
        calls = len(scene.project_calls)
        with pytest.raises(ValueError, match=r"^query 0: the goal lies in no region$"):
            sq.graphs(starts=np.array([[0.5, 0.5]]), goal_boxes=box, outside="snap")
        assert len(scene.project_calls) == calls


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
    """both entry points are one ``scene_entry``; every refusal of project_points stands in front of ``stage_start`` (so a refused call
    leaves the earlier list), the count of candidates is checked before the list is allocated, the call takes the row of
    locate_points, and read_projections needs a list that project_points made.  (test_gpu_point_project.py runs them.)"""
    src = open(os.path.join(build.CSRC, "polytope_lp.hip")).read()
    body = _body(src, "gcsadmm_scene_project_points")
    assert re.match(r"\{\s*return scene_entry\(s, \[&\]\(\) -> int \{", body)
    start = body.index("stage_start(s->have, CALL_LOCATE_POINTS);")
    for text in ("negative number of points or null points", "max_iter must not be negative", "point with a NaN or an inf coordinate", "is NaN or negative"):
        assert 0 < body.index(text) < start, text
    assert body.count("GCSADMM_ERR_BAD_ARG") == 4 and body.index("GCSADMM_ERR_BAD_ARG", start - 200) < start
    assert start < body.index("more than 2^31 - 1 candidates") < body.index("h.region.reserve(")
    assert body.index("h.projected = true;") < body.index("stage_finish(s->have, CALL_LOCATE_POINTS);")
    read = _body(src, "gcsadmm_scene_read_projections")
    assert re.match(r"\{\s*return scene_entry\(s, \[&\]\(\) -> int \{\s*NEED\(s, CALL_READ_HITS\);", read)
    assert read.index("if (!h.projected)") < read.index("to_host(")
    assert src.count("s->hits.projected = false;") == 2          # the two locate calls say which kind of list they leave
    # the header and the binding declare them
    header = open(os.path.join(build.ROOT, "include", "gcsadmm.h")).read()
    for name in ("gcsadmm_scene_project_points", "gcsadmm_scene_read_projections"):
        assert f"int {name}(gcsadmm_scene s," in header


def test_every_project_kernel_keeps_its_working_set_in_registers():
    res = {k: v for k, v in build.kernel_resources().items() if "project_" in k}
    solve = [k for k in res if "project_solve_kernel" in k]
    assert len(solve) == 8 and len(res) == 24, sorted(res)          # N = 1 .. 8; the list kernel in its two passes
    for k, v in res.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (k, v)


def test_the_core_runs_clean_under_the_sanitizers():
    """a stand-alone program (its own main) on a crafted scene, compiled with -fsanitize=address,undefined and run here"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    exe = build_library(os.path.join(build.ROOT, "build", "project_sanitize"), hostemu_lib.sources([("project_sanitize.cpp", [])]),
                        flags=hostemu_lib.FLAGS + ["-ffp-contract=off"] + san, link_flags=san)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok" and p.stderr == "", (p.returncode, p.stdout, p.stderr)


def test_report_the_worst_figures():
    """what the tests above measured (run the whole file): profiles/project/README.md records them"""
    print("worst feasibility / allowance %.3g, worst gap / scale %.3g, most iterations %d" % (WORST["feasibility"], WORST["gap"], WORST["iterations"]))
