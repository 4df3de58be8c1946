"""Case families for the polytope LPs (csrc/polytope_lp.hip, polytope_lp_core.h), the HiGHS reference for them, and the ONE contract
that the host build (tests/hostemu/lp_emu.cpp) and the device kernels are both held to.

Families (deterministic, seeded; each gives ``polys``, the pairs to decide, and a per-polytope ``width`` used for margins):
  * ``mixed_rows(n)``   130 polytopes (two full wavefronts and a tail of two) with their own row counts, widths 0.05-5, offsets 0 / 30 /
                        300 / 3e3, one with non-unit normals, one with every row three times, two point boxes;
  * ``scales(n)``       20 polytopes each at width 1e-3, 1, 1e2, 1e4 around the origin, and the width-1 scene again 3e4 away;
  * ``touching(n)``     boxes sharing a face or a corner, or 1e-5 apart, point boxes, one box around everything -- known answers, decided
                        from the centres and from no start point, at offsets 0 and 300;
  * ``polygon_limit()`` regular polygons with 79 and 159 sides (the largest overlap / centre LPs that fit LDS), analytic answers.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from gcs_admm_amd.graph import convert_pt_to_polytope   # noqa: E402
from hostemu_lib import emu_library     # noqa: E402
from gcs_admm_amd.scene import SWEEP_PAD                 # noqa: E402
from oracle import polytope_oracle as PO                 # noqa: E402

EMU_SRC = os.path.join(ROOT, "tests", "hostemu", "lp_emu.cpp")

TOL = 1e-9                          # the pipeline's overlap tolerance (build_graph_device)
NEWTON_MAX = 25                     # Newton steps of a centre or bounds LP (host build; the bound of the width-1 ball-LP test)
BOX_SHORTFALL = 0.1 * SWEEP_PAD     # a box may be too small by a tenth of the sweep's pad, no more
PAIRS_PER_N = 600                   # HiGHS decides each sampled pair once: keeps a test to a few seconds


def random_polytope(rng, n, m, centre, scale):
    """m random half-spaces at distance ~scale around `centre` plus a bounding box (always bounded)."""
    A = rng.normal(size=(m, n)); A /= np.linalg.norm(A, axis=1)[:, None]
    b = A @ centre + scale * rng.uniform(0.3, 1.0, size=m)
    A = np.vstack([A, np.eye(n), -np.eye(n)])
    b = np.hstack([b, centre + 2 * scale, -(centre - 2 * scale)])
    return A, b


def box(lo, hi):
    lo = np.asarray(lo, float); hi = np.asarray(hi, float)
    n = len(lo)
    return np.vstack([np.eye(n), -np.eye(n)]), np.hstack([hi, -lo])


@dataclass
class Family:
    name: str
    n: int
    polys: list
    width: np.ndarray                       # [P] the size of each polytope: margins are stated relative to it
    pa: np.ndarray
    pb: np.ndarray
    expected: np.ndarray | None = None      # known answers of the pairs (then no pair is skipped and HiGHS is not asked)
    starts: tuple = ("centres",)            # start points of the overlap LPs: the centres, and / or none
    analytic: dict = field(default_factory=dict)   # {p: (centre, radius, lo, hi)} where known in closed form
    origin: np.ndarray | None = None        # [P, n] the offset each polytope was generated at (reference(): HiGHS solves around it)


# ------------------------------------------------------------------------------------------- families
def _sample_pairs(rng, pa, pb, k):
    if len(pa) > k:
        sel = np.sort(rng.choice(len(pa), k, replace=False))
        pa, pb = pa[sel], pb[sel]
    return pa.astype(np.int32), pb.astype(np.int32)


MIXED_P = 130
MIXED_OFFSETS = (0.0, 30.0, 300.0, 3e3)
MIXED_SCALED, MIXED_TRIPLED, MIXED_POINTS = 5, 6, (7, 8)
# the overlap LP of a pair holds the rows of both polytopes in LDS: 79 rows each at the most (polygon_limit), so the polytope whose
# rows are repeated three times has at most 26 distinct ones
MIXED_TRIPLED_ROWS = 79 // 3


@functools.lru_cache(maxsize=None)
def mixed_rows(n, P=MIXED_P, seed=100):
    rng = np.random.default_rng(seed + n)
    direction = np.where(np.arange(n) % 2 == 0, 1.0, -0.8)
    spread = 2.2 * n ** -0.5                      # neighbours of one offset group sit this far apart: about half the pairs overlap
    polys, width, centres = [], np.empty(P), np.empty((P, n))
    origin = np.array([MIXED_OFFSETS[p % 4] * direction for p in range(P)])
    for p in range(P):
        wd = 0.05 * 100.0 ** rng.uniform()        # 0.05 .. 5, log-uniform
        c = MIXED_OFFSETS[p % 4] * direction + spread * rng.uniform(-1, 1, n)
        m = int(rng.integers(1, 3 * n + 4))       # 1 .. 3n + 3 random rows of its own
        if p == MIXED_TRIPLED:
            m = min(m, MIXED_TRIPLED_ROWS - 2 * n)
        A, b = random_polytope(rng, n, m, c, wd)
        if p == MIXED_SCALED:                     # non-unit normals
            f = 10.0 ** rng.uniform(-3, 3, len(b))
            A, b = A * f[:, None], b * f
        if p == MIXED_TRIPLED:                    # every row three times
            A, b = np.repeat(A, 3, axis=0), np.repeat(b, 3)
        if p in MIXED_POINTS:                     # the reference's point vertices, inside the polytope four places earlier
            c = centres[p - 4] + 0.05 * width[p - 4] * rng.uniform(-1, 1, n)
            A, b = convert_pt_to_polytope(c)
            wd = 1e-6
        polys.append((A, b)); width[p] = wd; centres[p] = c
    pa, pb = np.triu_indices(P, 1)
    same = (pa % 4) == (pb % 4)                   # pairs inside one offset group, and a few across groups (all disjoint)
    ia, ib = _sample_pairs(rng, pa[same], pb[same], PAIRS_PER_N - 40)
    ca, cb = _sample_pairs(rng, pa[~same], pb[~same], 40 - len(MIXED_POINTS))
    qa = np.array([q - 4 for q in MIXED_POINTS], np.int32); qb = np.array(MIXED_POINTS, np.int32)
    return Family("mixed_rows", n, polys, width, np.concatenate([ia, ca, qa]), np.concatenate([ib, cb, qb]), origin=origin)


SCALES = ((1e-3, 0.0), (1.0, 0.0), (1e2, 0.0), (1e4, 0.0), (1.0, 3e4))   # (width, offset); the last is the second scene again, far away
SCALES_P = 20


@functools.lru_cache(maxsize=None)
def scales(n, seed=200):
    polys, width, pa, pb, origin = [], [], [], [], []
    direction = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    for s, (wd, off) in enumerate(SCALES):
        rng = np.random.default_rng(seed + 10 * n + (1 if off else s))    # the far scene repeats the draws of the width-1 scene
        for _ in range(SCALES_P):
            A, b = random_polytope(rng, n, n + 4, wd * rng.uniform(-1, 1, n), wd * rng.uniform(0.4, 1.2))
            polys.append((A, b + A @ (off * direction))); width.append(wd); origin.append(off * direction)
        a, b_ = np.triu_indices(SCALES_P, 1)
        a, b_ = _sample_pairs(np.random.default_rng(seed + s), a, b_, PAIRS_PER_N // len(SCALES))
        pa.append(a + s * SCALES_P); pb.append(b_ + s * SCALES_P)
    return Family("scales", n, polys, np.array(width), np.concatenate(pa).astype(np.int32), np.concatenate(pb).astype(np.int32),
                  origin=np.array(origin))


TOUCHING_OFFSETS = (0.0, 300.0)


@functools.lru_cache(maxsize=None)
def touching(n):
    """unit box 0; 1 shares a face with it; 2 is 1e-5 away along one axis; 3 shares a corner; 4 is 1e-5 away from the corner along
    every axis; 5 a point box inside 0; 6 a point box outside 0; 7 the 100-wide box around everything.  Closed sets: touching counts."""
    g = 1e-5
    one, zero = np.ones(n), np.zeros(n)
    e0 = np.zeros(n); e0[0] = 1.0
    polys, width, pa, pb, exp, origin = [], [], [], [], [], []
    pairs = [(0, 1, 1), (0, 2, 0), (0, 3, 1), (0, 4, 0), (0, 5, 1), (0, 6, 0), (5, 7, 1), (6, 7, 1), (1, 2, 1), (0, 7, 1), (3, 4, 1), (1, 3, 1),
             (2, 4, 0 if n > 1 else 1), (5, 6, 0)]
    for k, off in enumerate(TOUCHING_OFFSETS):
        o = off * one
        far = np.full(n, 3.0); far[0] = 1.5
        polys += [box(o, o + 1), box(o + e0, o + e0 + 1), box(o + (1 + g) * e0, o + e0 + 1), box(o + 1, o + 2), box(o + 1 + g, o + 2),
                  convert_pt_to_polytope(o + 0.5), convert_pt_to_polytope(o + far), box(o - 50, o + 50)]
        width += [1, 1, 1, 1, 1, 1e-6, 1e-6, 100]; origin += [o] * 8
        for a, b, f in pairs:
            pa.append(a + 8 * k); pb.append(b + 8 * k); exp.append(f)
    # pair (2, 4): [1+g, 2] x [0, 1]^(n-1) against [1+g, 2]^n are g apart along the second axis; in n = 1 they are the same interval
    return Family("touching", n, polys, np.array(width, float), np.array(pa, np.int32), np.array(pb, np.int32),
                  expected=np.array(exp, np.uint8), starts=("centres", "none"), origin=np.array(origin))


def regular_polygon(m, centre, phase=0.1):
    """(A, b, lo, hi) of the regular m-gon of inradius 1 around `centre`"""
    th = phase + 2 * np.pi * np.arange(m) / m
    A = np.stack([np.cos(th), np.sin(th)], axis=1)
    v = np.asarray(centre) + np.stack([np.cos(th + np.pi / m), np.sin(th + np.pi / m)], axis=1) / np.cos(np.pi / m)
    return A, A @ np.asarray(centre) + 1.0, v.min(axis=0), v.max(axis=0)


POLYGON_SIDES = (79, 159)     # the most rows per polytope that an overlap LP (2 m + 1 rows) and a centre LP (m + 1 rows) fit into LDS


@functools.lru_cache(maxsize=None)
def polygon_limit():
    """polytopes 0-2: 79-gons (1 overlaps 0, 2 is clear of both); 3-4: 159-gons.  Centre, radius 1 and box in closed form; the pairs
    follow from the distance of the centres against the in- and circumradius (2 < d: apart beyond the circumradii; d < 2: the incircles meet)."""
    c = np.array([3.0, -2.0])
    cs = [c, c + [1.2, 0.5], c + [-2.0, 1.7], c + [40.0, 0.0], c + [41.0, 0.3]]
    polys, analytic = [], {}
    for p, cc in enumerate(cs):
        A, b, lo, hi = regular_polygon(POLYGON_SIDES[0] if p < 3 else POLYGON_SIDES[1], cc)
        polys.append((A, b)); analytic[p] = (cc, 1.0, lo, hi)
    return Family("polygon_limit", 2, polys, np.ones(len(cs)), np.array([0, 0, 1, 3], np.int32), np.array([1, 2, 2, 4], np.int32),
                  expected=np.array([1, 0, 0, 1], np.uint8), analytic=analytic)


def polygon_with_rows(m, centre=(3.0, -2.0)):
    A, b, _, _ = regular_polygon(m, np.asarray(centre, float))
    return A, b


FAMILIES = {"mixed_rows": mixed_rows, "scales": scales, "touching": touching}


def family(name, n):
    return polygon_limit() if name == "polygon_limit" else FAMILIES[name](n)


# ------------------------------------------------------------------------------------------- reference (HiGHS), computed once
@dataclass
class Reference:
    radius: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    rstar: np.ndarray | None      # inscribed radius of the intersection per pair (None where the answers are known)


def _around(A, b, origin):
    """the rows of A x <= b in the coordinates x - origin, formed in extended precision (the same polytope to the last bit of b)"""
    return A, np.asarray(b.astype(np.longdouble) - A.astype(np.longdouble) @ origin.astype(np.longdouble), np.float64)


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """HiGHS (oracle/polytope_oracle.py) on every polytope and pair of the family, solved in coordinates around the offset the polytope
    was generated at: given rows 3e4 from the origin as they stand, HiGHS's simplex returned a radius 3e-6 too large with a centre
    whose own ball was 2e-5 smaller (its feasibility tolerances act on the unshifted right-hand sides) -- further off than the
    contract allows the code under test to be.  The radius it returns is checked against the ball its own centre has."""
    fam = family(name, n)
    P = len(fam.polys)
    rad = np.empty(P); lo = np.empty((P, fam.n)); hi = np.empty((P, fam.n))
    for p, (A, b) in enumerate(fam.polys):
        if p in fam.analytic:
            _, rad[p], lo[p], hi[p] = fam.analytic[p]
        else:
            A0, b0 = _around(A, b, fam.origin[p])
            x, rad[p] = PO.chebyshev(A0, b0)
            own = ((b0 - A0 @ x) / np.linalg.norm(A0, axis=1)).min()
            assert abs(own - rad[p]) <= 1e-9 * max(1.0, abs(rad[p])), f"reference: HiGHS radius {rad[p]!r} of {name} n={n} polytope {p}, its centre has {own!r}"
            lo[p], hi[p] = PO.bounding_box(A0, b0)
            lo[p] += fam.origin[p]; hi[p] += fam.origin[p]
    rstar = None
    if fam.expected is None:
        rstar = np.array([PO.overlap_radius(*_around(*fam.polys[i], fam.origin[i]), *_around(*fam.polys[j], fam.origin[i]))
                          for i, j in zip(fam.pa, fam.pb)])
    for a in (rad, lo, hi, rstar):
        if a is not None:
            a.setflags(write=False)
    return Reference(rad, lo, hi, rstar)


# ------------------------------------------------------------------------------------------- the host build
def load_lp_emu():
    """tests/hostemu/lp_emu.cpp against csrc/polytope_lp_core.h, rebuilt when a source changes"""
    return emu_library("lpemu")


class HostLP:
    """The interface of gcs_admm_amd.scene.PolytopeScene (centers / bounds / overlaps) on the host build, one LP per call;
    keeps the Newton counts (``it_c`` [P], ``it_b`` [P, 2n], ``it_o`` [pairs]), which the device ABI does not export."""

    def __init__(self, lib, polys):
        self.lib = lib
        self.n = int(np.asarray(polys[0][0]).shape[1]); self.P = len(polys)
        self.ptr = np.zeros(self.P + 1, np.int32); self.ptr[1:] = np.cumsum([len(b) for _, b in polys])
        self.A = np.ascontiguousarray(np.vstack([np.asarray(a, float).reshape(-1, self.n) for a, _ in polys]))
        self.b = np.ascontiguousarray(np.hstack([np.asarray(bb, float).ravel() for _, bb in polys]))
        self.nrm = np.ascontiguousarray(np.linalg.norm(self.A, axis=1))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._csr = (C.c_int(self.n), C.c_int(self.P), vp(self.ptr), vp(self.A), vp(self.b), vp(self.nrm))
        self._centers = None

    def _ball(self, p, q, x0, early, tol):
        w = np.zeros(self.n + 1); it = C.c_int(-1)
        x0 = np.ascontiguousarray(x0, float) if x0 is not None else None
        st = self.lib.lp_emu_ball(*self._csr, C.c_int(int(p)), C.c_int(int(q)), x0.ctypes.data_as(C.c_void_p) if x0 is not None else None,
                                  C.c_int(early), C.c_double(tol), w.ctypes.data_as(C.c_void_p), C.byref(it))
        return st, w, it.value

    def centers(self):
        cen = np.empty((self.P, self.n)); rad = np.empty(self.P); st = np.empty(self.P, np.int32); self.it_c = np.empty(self.P, np.int32)
        for p in range(self.P):                     # gcsadmm_polytope_centers: no start point, no early exit, tol 0
            st[p], w, self.it_c[p] = self._ball(p, -1, None, 0, 0.0)
            cen[p], rad[p] = w[:self.n], w[self.n]
        self._centers = cen
        return cen, rad, st

    def bounds(self, centers=None):
        cen = np.ascontiguousarray(centers if centers is not None else (self._centers if self._centers is not None else self.centers()[0]))
        n = self.n
        lo = np.empty((self.P, n)); hi = np.empty((self.P, n)); st = np.empty((self.P, 2 * n), np.int32)
        self.it_b = np.empty((self.P, 2 * n), np.int32)
        out = C.c_double(0.0); it = C.c_int(-1)
        for p in range(self.P):
            x0 = cen[p].ctypes.data_as(C.c_void_p)
            for j in range(2 * n):                  # the status layout of bounds_kernel: [P][n][(min, max)]
                st[p, j] = self.lib.lp_emu_bound(*self._csr, C.c_int(p), x0, C.c_int(j >> 1), C.c_int(j & 1), C.byref(out), C.byref(it))
                (hi if j & 1 else lo)[p, j >> 1] = out.value
                self.it_b[p, j] = it.value
        return lo, hi, st

    def overlaps(self, pair_a, pair_b, tol=TOL, centers=None):
        T = len(pair_a)
        flags = np.zeros(T, np.uint8); st = np.zeros(T, np.int32); self.it_o = np.zeros(T, np.int32); self.r_o = np.zeros(T)
        for t, (p, q) in enumerate(zip(pair_a, pair_b)):
            st[t], w, self.it_o[t] = self._ball(p, q, centers[p] if centers is not None else None, 1, tol)
            self.r_o[t] = w[self.n]                 # the flag rule of ball_kernel
            flags[t] = 1 if st[t] == 1 else (0 if st[t] == 2 else (1 if w[self.n] >= -tol else 0))
        return flags, st


# ------------------------------------------------------------------------------------------- produce, then check
@dataclass
class Produced:
    cen: np.ndarray
    rad: np.ndarray
    st_c: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    st_b: np.ndarray
    flags: dict                    # {start: (flags, status)}
    it_c: np.ndarray | None = None
    it_b: np.ndarray | None = None


def produce(backend, fam):
    """centres -> boxes from them -> pair decisions from them (and from no start point where the family asks), on a HostLP or a PolytopeScene"""
    cen, rad, st_c = backend.centers()
    lo, hi, st_b = backend.bounds(cen)
    flags = {}
    for start in fam.starts:
        backend._centers = None                     # PolytopeScene.overlaps falls back to the centres it remembers
        flags[start] = backend.overlaps(fam.pa, fam.pb, TOL, cen if start == "centres" else None)
    return Produced(cen, rad, np.asarray(st_c), lo, hi, np.asarray(st_b).reshape(len(fam.polys), -1), flags,
                    getattr(backend, "it_c", None), getattr(backend, "it_b", None))


def check_contract(fam, out, ref, newton=True):
    """The contract of the three LP kinds on one family; raises AssertionError naming the first violation of each kind, returns the
    measured figures {radius_err_rel, ball_deficit, box_shortfall, box_excess, skipped, newton_centre, newton_bounds}."""
    n, P = fam.n, len(fam.polys)
    fig = {}
    # centres
    bad = np.nonzero(out.st_c != 0)[0]
    assert len(bad) == 0, f"{fam.name} n={n}: centre LP status {out.st_c[bad][:8].tolist()} for polytopes {bad[:8].tolist()} ({len(bad)} of {P})"
    assert np.all(np.isfinite(out.rad)) and np.all(np.isfinite(out.cen)), f"{fam.name} n={n}: non-finite centre with status 0"
    err = np.abs(out.rad - ref.radius)
    bound = 1e-9 * np.maximum(1.0, np.abs(ref.radius)) + 1e-11
    fig["radius_err_rel"] = float((err / np.maximum(1.0, np.abs(ref.radius))).max())
    p = int(np.argmax(err - bound))
    assert err[p] <= bound[p], f"{fam.name} n={n}: radius of polytope {p}: {out.rad[p]!r} against {ref.radius[p]!r}"
    deficit = np.empty(P)
    for p, (A, b) in enumerate(fam.polys):
        deficit[p] = out.rad[p] - ((b - A @ out.cen[p]) / np.linalg.norm(A, axis=1)).min()
    fig["ball_deficit"] = float((deficit / np.maximum(1.0, fam.width)).max())
    p = int(np.argmax(deficit - 1e-9 * np.maximum(1.0, fam.width)))
    assert deficit[p] <= 1e-9 * max(1.0, fam.width[p]), f"{fam.name} n={n}: the point returned for polytope {p} has no ball of radius r around it ({deficit[p]:.3e} short)"
    # boxes
    bad = np.argwhere(out.st_b != 0)
    assert len(bad) == 0, f"{fam.name} n={n}: bounds LP status != 0 for (polytope, side) {bad[:8].tolist()} ({len(bad)} of {P * 2 * n})"
    assert np.all(np.isfinite(out.lo)) and np.all(np.isfinite(out.hi)), f"{fam.name} n={n}: non-finite box with status 0"
    short = np.maximum(out.lo - ref.lo, ref.hi - out.hi)            # > 0: the box is too small on that side
    fig["box_shortfall"] = float(short.max()); fig["box_excess"] = float((-np.minimum(out.lo - ref.lo, ref.hi - out.hi)).max())
    p, k = np.unravel_index(np.argmax(short), short.shape)
    assert short[p, k] <= BOX_SHORTFALL, f"{fam.name} n={n}: box of polytope {p} too small by {short[p, k]:.3e} on axis {k}"
    for dev, rf, side in ((out.lo, ref.lo, "lo"), (out.hi, ref.hi, "hi")):
        d = np.abs(dev - rf) - 1e-8 * np.maximum(1.0, np.abs(rf))
        p, k = np.unravel_index(np.argmax(d), d.shape)
        assert d[p, k] <= 0, f"{fam.name} n={n}: {side}[{p}, {k}] = {dev[p, k]!r} against {rf[p, k]!r}"
    # overlaps
    pw = np.minimum(fam.width[fam.pa], fam.width[fam.pb])
    if fam.expected is not None:
        want, keep = fam.expected.astype(bool), np.ones(len(fam.pa), bool)
    else:
        want, keep = ref.rstar > 0, np.abs(ref.rstar) >= 1e-6 * pw
    fig["skipped"] = int((~keep).sum())
    assert (~keep).sum() <= 0.1 * len(keep), f"{fam.name} n={n}: {(~keep).sum()} of {len(keep)} pairs have no margin"
    for start, (flags, st) in out.flags.items():
        st = np.asarray(st); flags = np.asarray(flags)
        bad = np.nonzero(st < 0)[0]
        assert len(bad) == 0, f"{fam.name} n={n} start={start}: overlap LP status -1 for pairs {[(int(fam.pa[t]), int(fam.pb[t])) for t in bad[:8]]} ({len(bad)})"
        bad = np.nonzero((flags.astype(bool) != want) & keep)[0]
        assert len(bad) == 0, (f"{fam.name} n={n} start={start}: wrong decisions {[(int(fam.pa[t]), int(fam.pb[t]), int(flags[t]), int(st[t])) for t in bad[:8]]}"
                               f" ({len(bad)}); r* = {None if ref.rstar is None else ref.rstar[bad[:8]].tolist()}")
    # Newton counts (the host build only)
    if newton:
        assert out.it_c is not None and out.it_b is not None, "Newton counts come from the host build"
        fig["newton_centre"] = int(out.it_c.max()); fig["newton_bounds"] = int(out.it_b.max())
        assert out.it_c.max() <= NEWTON_MAX, f"{fam.name} n={n}: centre LP of polytope {int(np.argmax(out.it_c))} took {out.it_c.max()} Newton steps"
        assert out.it_b.max() <= NEWTON_MAX, f"{fam.name} n={n}: a bounds LP of polytope {int(np.argmax(out.it_b.max(axis=1)))} took {out.it_b.max()} Newton steps"
    return fig


def check_against_host(fam, dev, host):
    """the device kernels against the host build of the same core on the same inputs: statuses and flags equal, radii and boxes within
    1e-9 relative (the two builds contract multiply-adds differently, so not bitwise)"""
    n = fam.n
    assert np.array_equal(dev.st_c, host.st_c), f"{fam.name} n={n}: centre statuses differ at {np.nonzero(dev.st_c != host.st_c)[0][:8].tolist()}"
    assert np.array_equal(dev.st_b, host.st_b), f"{fam.name} n={n}: bounds statuses differ at {np.argwhere(dev.st_b != host.st_b)[:8].tolist()}"
    for name, a, b in (("radius", dev.rad, host.rad), ("lo", dev.lo, host.lo), ("hi", dev.hi, host.hi)):
        d = np.abs(a - b) - 1e-9 * np.maximum(1.0, np.abs(b))
        i = np.unravel_index(np.argmax(d), d.shape)
        assert d[i] <= 0, f"{fam.name} n={n}: {name}{list(map(int, i))}: device {a[i]!r}, host build {b[i]!r}"
    for start in fam.starts:
        (fd, sd), (fh, sh) = dev.flags[start], host.flags[start]
        assert np.array_equal(fd, fh), f"{fam.name} n={n} start={start}: flags differ at pairs {np.nonzero(np.asarray(fd) != np.asarray(fh))[0][:8].tolist()}"
        assert np.array_equal(sd, sh), f"{fam.name} n={n} start={start}: overlap statuses differ at pairs {np.nonzero(np.asarray(sd) != np.asarray(sh))[0][:8].tolist()}"
