"""A stand-in for scene.PolytopeScene that reports LP failures, and the four boxes it knows: for the tests of what graph construction
does with an LP status (test_graph.py, test_scene_resident.py).  No GPU needed."""
import numpy as np


def four_boxes():
    A = np.vstack([np.eye(2), -np.eye(2)])
    As = {k: A for k in range(4)}
    bs = {0: np.array([1.0, 1.0, 0.0, 0.0]), 1: np.array([2.0, 1.0, -0.9, 0.0]),      # 0-1 overlap, 1-2 overlap, 3 apart
          2: np.array([3.0, 1.0, -1.9, 0.0]), 3: np.array([9.0, 9.0, -8.0, -8.0])}
    return As, bs


class FakeScene:
    """the interface of scene.PolytopeScene on ``four_boxes``; mode: "ok", or which LPs fail: "center" (region 2), "bounds" (one side
    of a box), "overlap" (every pair, with the wrong flag)"""
    def __init__(self, mode): self.mode = mode
    def centers(self):
        cen = np.array([[0.5, 0.5], [1.45, 0.5], [2.45, 0.5], [8.5, 8.5]])
        st = np.zeros(4, np.int32)
        if self.mode == "center": st[2] = -1
        return cen, np.full(4, 0.4), st
    def bounds(self, cen):
        lo = np.array([[0, 0], [0.9, 0], [1.9, 0], [8, 8]], float); hi = np.array([[1, 1], [2, 1], [3, 1], [9, 9]], float)
        st = np.zeros((4, 2, 2), np.int32)
        if self.mode == "bounds":          # region 1's upper x bound stopped early at an interior point
            hi[1, 0] = 1.5; st[1, 0, 1] = -1
        return lo, hi, st
    def overlaps(self, pa, pb, tol, cen):
        flags = np.array([1 if (min(a, b), max(a, b)) in {(0, 1), (1, 2)} else 0 for a, b in zip(pa, pb)], np.uint8)
        st = np.zeros(len(pa), np.int32)
        if self.mode == "overlap":         # every LP "failed" and reports the wrong answer
            st[:] = -1; flags[:] = 1 - flags
        return flags, st
