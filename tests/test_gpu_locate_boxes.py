"""locate_box_kernel on the device (gcsadmm_scene_locate_boxes / read_hits through scene.DeviceScene.locate_boxes) against its host
build byte for byte, on the scenes and boxes of test_locate_boxes.py, which holds that build to polytopes_overlap and graph_from_sets;
zero boxes, the refusals, and locate_points around a locate_boxes call."""
import ctypes as C

import numpy as np
import pytest

import locate_box_cases as bxc
import locate_cases as L
from gcs_admm_amd import scene as sc
from gcs_admm_amd.abi import GcsAdmmError

pytestmark = pytest.mark.gpu

SIZES = (1, 65, 600)          # one region; a stride and one; three chunks of LOCATE_CHUNK = 256 with a partial last one: the scan across chunks


def same_hits(got, want, what):
    for g, w, f in zip(got, want, ("hit_ptr", "hit_region", "hit_class")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, f)


@pytest.mark.parametrize("n", L.DIMS)
@pytest.mark.parametrize("kind,offset", L.FAMILIES)
def test_box_kernel_equals_the_host_build(kind, offset, n):
    """the three arrays equal the host build's for 1 and 12 boxes, and a second call returns them again"""
    assert max(SIZES) > 2 * L.CHUNK
    for P in SIZES:
        lo, hi = bxc.boxes(kind, n, P, offset, 12)
        with sc.DeviceScene(L.regions(kind, n, P, offset)) as scene:
            for Q in (1, 12):
                want = bxc.family_hits(kind, n, P, offset, Q)
                same_hits(scene.locate_boxes(lo[:Q], hi[:Q]), want, (P, Q))
            same_hits(scene.locate_boxes(lo, hi), want, (P, "second call"))
            assert P < 65 or len(want[1]) > 0


def test_sound_cases_crafted_and_interior_boxes_on_the_device():
    """the inputs of the host tests' soundness, crafted and interior-box checks give the host build's lists on the device too"""
    names, polys, lo, hi, expect, _ = bxc.crafted()
    with sc.DeviceScene(polys) as scene:
        hits = scene.locate_boxes(lo, hi)
        same_hits(hits, bxc.emu_locate_boxes(polys, lo, hi), "crafted")
        M = L.dense(hits, len(lo), len(polys))
        for (q, name), cls in expect.items():
            assert M[q, names.index(name)] == cls, (q, name)
        empty = scene.locate_boxes(np.zeros((0, 2)), np.zeros((0, 2)))                  # zero boxes
        assert empty[0].tolist() == [0] and len(empty[1]) == len(empty[2]) == 0
    for kind, n in (("polytopes", 3), ("scaled", 8)):
        for P, mk in ((40, lambda p: bxc.boxes(kind, n, 40, 0.0, 12)), (65, lambda p: bxc.interior_boxes(p, n)[:2])):
            polys = L.regions(kind, n, P, 0.0)
            lo, hi = mk(polys)
            with sc.DeviceScene(polys) as scene:
                same_hits(scene.locate_boxes(lo, hi), bxc.emu_locate_boxes(polys, lo, hi), (kind, n, P))


def test_refusals_leave_the_list_and_locate_points_is_unchanged():
    polys = L.regions("polytopes", 2, 130)
    pts = L.points("polytopes", 2, 130)[:5]
    lo, hi = bxc.boxes("polytopes", 2, 130, 0.0, 5)
    with sc.DeviceScene(polys) as scene:
        points_before = scene.locate(pts)
        same_hits(points_before, L.emu_locate(polys, pts), "points before")
        want = bxc.emu_locate_boxes(polys, lo, hi)
        same_hits(scene.locate_boxes(lo, hi), want, "boxes")
        bad = hi.copy(); bad[2, 1] = lo[2, 1] - 1e-3
        with pytest.raises(GcsAdmmError, match=r"lo > hi.*status 1"):
            scene.locate_boxes(lo, bad)
        for value in (np.nan, np.inf, -np.inf):
            for side in (0, 1):
                l, h = lo.copy(), hi.copy()
                (l, h)[side][3, 0] = value
                with pytest.raises(GcsAdmmError, match=r"NaN or an inf.*status 1"):
                    scene.locate_boxes(l, h)
        for tol in (-1e-9, np.nan, np.inf):
            with pytest.raises(GcsAdmmError, match=r"tol must be finite.*status 1"):
                scene.locate_boxes(lo, hi, tol=tol)
        num = C.c_int64(-7)
        for args in ((-1, lo.ctypes.data, hi.ctypes.data), (5, None, hi.ctypes.data), (5, lo.ctypes.data, None)):
            with pytest.raises(GcsAdmmError, match=r"negative number of boxes or null bounds.*status 1"):
                scene._call("gcsadmm_scene_locate_boxes", *args, 1e-9, C.addressof(num))
        assert num.value == -7
        # the refused calls took nothing: the list made before them is still there
        got = (np.zeros(6, np.int64), np.zeros(len(want[1]), np.int32), np.zeros(len(want[2]), np.uint8))
        scene._call("gcsadmm_scene_read_hits", *(a.ctypes.data for a in got))
        same_hits(got, want, "after the refusals")
        # locate_points gives after a locate_boxes call what it gave before it, and the other way round
        same_hits(scene.locate(pts), points_before, "points after")
        same_hits(scene.locate_boxes(lo, hi), want, "boxes again")
    from gcs_admm_amd import abi
    assert abi.load_library().gcsadmm_scene_locate_boxes(None, 0, None, None, 1e-9, None) == 1          # a null scene is a bad argument
