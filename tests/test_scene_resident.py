"""The resident scene of graph construction, the parts that need no GPU: the host build of the device broad phase
(tests/hostemu/sweep_emu.cpp compiles csrc/box_sweep_core.h, the code sweep_kernel runs, with the lanes one after the other) against
``scene.candidate_pairs`` element for element; the scan that places the boxes' segments; and ``build_graph_arrays_device`` on a
stand-in scene that reports LP failures.  The kernels themselves: test_gpu_scene_resident.py."""
import ctypes as C

import numpy as np
import pytest

import sweep_cases as S
from scene_fakes import FakeScene, four_boxes as _four_boxes
from gcs_admm_amd import scene as sc


@pytest.fixture(scope="module")
def emu():
    return S.load_sweep_emu()


def _same_list(emu, lo, hi, pad):
    pa, pb = S.emu_pairs(emu, lo, hi, pad)
    ra, rb = sc.candidate_pairs(lo, hi, pad)
    assert pa.dtype == ra.dtype == np.int32
    assert np.array_equal(pa, ra) and np.array_equal(pb, rb), (len(pa), len(ra))
    assert np.all(pa < pb)
    return pa, pb


@pytest.mark.parametrize("P", S.SIZES)
@pytest.mark.parametrize("n", S.DIMS)
def test_host_build_of_the_sweep_equals_candidate_pairs(emu, n, P):
    lo, hi = S.boxes(n, P)
    for pad in S.pads():
        pa, _ = _same_list(emu, lo, hi, pad)
        S.check_share(P, len(pa))
    if P == 1000:       # windows of several 64-lane strides: the order across strides is under test
        order = np.argsort(lo[:, 0], kind="stable")
        end = np.searchsorted(lo[order, 0], hi[order, 0], side="right")
        assert (end - np.arange(P) - 1 > 64).sum() >= 100


@pytest.mark.parametrize("pad_index", [0, 1])
def test_host_build_of_the_sweep_on_ties_infinities_and_touching_boxes(emu, pad_index):
    pad = S.pads()[pad_index]
    lo, hi = S.extras(pad)
    pa, pb = _same_list(emu, lo, hi, pad)
    S.check_share(130, len(pa))
    S.check_extras(pa, pb)
    assert set(zip(pa.tolist(), pb.tolist())) == S.brute_force(lo, hi, pad)
    # the tie order is numpy's: the box with lo = -0.0 is swept after the +0.0 boxes before it, so as the first box of a pair it
    # comes where the stable order puts it (a sort that tells -0.0 from +0.0 gives the same set in another order)
    lo2 = lo.copy(); lo2[S.TIES[7], 0] = -1e-300
    qa, qb = sc.candidate_pairs(lo2, hi, pad)
    assert set(zip(qa.tolist(), qb.tolist())) == set(zip(pa.tolist(), pb.tolist())) and not np.array_equal(qa, pa)


@pytest.mark.parametrize("n", S.DIMS)
def test_host_build_of_the_sweep_equals_brute_force(emu, n):
    lo, hi = S.boxes(n, 130)
    for pad in S.pads():
        pa, pb = S.emu_pairs(emu, lo, hi, pad)
        ref = S.brute_force(lo, hi, pad)
        assert set(zip(pa.tolist(), pb.tolist())) == ref and len(pa) == len(ref)


def test_host_build_of_the_sweep_nothing_and_everything(emu):
    lo = np.arange(65, dtype=float)[:, None] * np.array([[2.0, 0.0]]); hi = lo + 1.0        # 65 disjoint boxes in a row
    assert len(_same_list(emu, lo, hi, S.pads()[1])[0]) == 0
    lo = np.zeros((300, 3)); hi = np.ones((300, 3))                                          # 300 identical boxes: every pair
    pa, pb = _same_list(emu, lo, hi, 0.0)
    ta, tb = np.triu_indices(300, 1)
    assert np.array_equal(pa, ta) and np.array_equal(pb, tb)


def test_scan_reports_a_total_beyond_int32_without_overflow(emu):
    count = np.full(70000, 69999, np.int32)
    offset = np.empty(70000, np.int64); total = C.c_longlong(0)
    assert emu.sweep_emu_scan(count.ctypes.data, 70000, offset.ctypes.data, C.addressof(total)) == 0
    assert total.value == 70000 * 69999 > 2 ** 31 - 1
    assert np.array_equal(offset, np.arange(70000, dtype=np.int64) * 69999)
    count[:] = 30000                                                                         # 2.1e9: just inside
    assert emu.sweep_emu_scan(count.ctypes.data, 70000, offset.ctypes.data, C.addressof(total)) == 1 and total.value == 2_100_000_000
    assert emu.sweep_emu_scan(None, 0, None, C.addressof(total)) == 1 and total.value == 0
    assert emu.sweep_emu_pairs(9, 1, None, None, 0.0, None, None, 0) == -99                  # n outside 1..8 is not dispatched


# ------------------------------------------------------------------------------------------- the array pipeline on a stand-in scene
class FakeDeviceScene:
    """the interface of scene.DeviceScene with the failures of scene_fakes.FakeScene: a centre LP, one side of a box, every
    overlap LP (with the wrong flag)"""

    def __init__(self, mode):
        self.mode = mode
        self.closed = False

    def centers(self):
        cen = np.array([[0.5, 0.5], [1.45, 0.5], [2.45, 0.5], [8.5, 8.5]])
        st = np.zeros(4, np.int32)
        if self.mode == "center":
            st[2] = -1
        return cen, np.full(4, 0.4), st

    def bounds(self):
        lo = np.array([[0, 0], [0.9, 0], [1.9, 0], [8, 8]], float); hi = np.array([[1, 1], [2, 1], [3, 1], [9, 9]], float)
        st = np.zeros((4, 4), np.int32)
        if self.mode == "bounds":          # region 1's upper x bound stopped early at an interior point: the device opens that side
            hi[1, 0] = np.inf; st[1, 1] = -1
        self.lo, self.hi = lo, hi
        return lo, hi, st

    def candidate_pairs(self, pad=sc.SWEEP_PAD):
        self.pa, self.pb = sc.candidate_pairs(self.lo, self.hi, pad)
        return len(self.pa)

    def overlaps(self, tol):
        self.flags = np.array([1 if (a, b) in {(0, 1), (1, 2)} else 0 for a, b in zip(self.pa.tolist(), self.pb.tolist())], np.uint8)
        self.st = np.zeros(len(self.pa), np.int32)
        if self.mode == "overlap":         # every LP "failed" and reports the wrong answer
            self.st[:] = -1; self.flags[:] = 1 - self.flags
        return int(self.flags.sum()), int((self.st < 0).sum())

    def pairs(self):
        return self.pa, self.pb, self.flags, self.st

    def close(self):
        self.closed = True


@pytest.mark.parametrize("mode", ["ok", "bounds", "overlap"])
def test_array_pipeline_acts_on_lp_status(mode):
    from gcs_admm_amd.graph import build_graph
    As, bs = _four_boxes()
    V, E_ref, I_in_ref, I_out_ref = build_graph(As, bs)
    polys = [(As[v], bs[v]) for v in V]
    stats = {}
    fake = FakeDeviceScene(mode)
    tail, head, cen = sc.build_graph_arrays_device(polys, scene=fake, stats=stats)
    assert tail.dtype == head.dtype == np.int32
    assert [(V[t], V[h]) for t, h in zip(tail, head)] == E_ref
    assert cen.shape == (4, 2) and not fake.closed            # a scene that was handed in stays open
    assert set(stats) == {"bounds_opened", "overlaps_redone_on_host", "candidate_pairs"}
    assert stats["bounds_opened"] == (1 if mode == "bounds" else 0)
    assert stats["overlaps_redone_on_host"] == (stats["candidate_pairs"] if mode == "overlap" else 0)
    assert stats["candidate_pairs"] == 2                      # 0-1 and 1-2; the opened side of region 1 reaches region 3 in x only
    # the same entry point in host mode, on the stand-in for a PolytopeScene: the same edges and the same three counts
    host_stats = {}
    tail_h, head_h, cen_h = sc.build_graph_arrays_device(polys, scene=FakeScene(mode), stats=host_stats, broad_phase="host")
    assert tail_h.dtype == head_h.dtype == np.int32
    assert np.array_equal(tail_h, tail) and np.array_equal(head_h, head) and np.array_equal(cen_h, cen)
    assert host_stats == stats
    # the keyed front end on the same scene: the reference's lists
    _, E, I_in, I_out, _ = sc.build_graph_device(As, bs, scene=FakeDeviceScene(mode), broad_phase="device")
    assert E == E_ref and I_in == I_in_ref and I_out == I_out_ref


def test_array_pipeline_refuses_a_failed_centre():
    As, bs = _four_boxes()
    As = {f"r{k}": v for k, v in As.items()}; bs = {f"r{k}": v for k, v in bs.items()}
    with pytest.raises(sc.GcsAdmmError, match=r"centre LP did not converge for regions \['r2'\]"):     # by key, as the host path says it
        sc.build_graph_device(As, bs, scene=FakeDeviceScene("center"), broad_phase="device")
    with pytest.raises(sc.GcsAdmmError, match=r"centre LP did not converge for regions \[2\]"):
        sc.build_graph_arrays_device([(As[v], bs[v]) for v in As], scene=FakeDeviceScene("center"))
    # host mode says the same, by key and by index
    with pytest.raises(sc.GcsAdmmError, match=r"centre LP did not converge for regions \['r2'\] \(of 1\)"):
        sc.build_graph_arrays_device([(As[v], bs[v]) for v in As], scene=FakeScene("center"), names=list(As), broad_phase="host")
    with pytest.raises(sc.GcsAdmmError, match=r"centre LP did not converge for regions \[2\] \(of 1\)"):
        sc.build_graph_arrays_device([(As[v], bs[v]) for v in As], scene=FakeScene("center"), broad_phase="host")


def test_broad_phase_default_is_the_host_sweep():
    import inspect
    assert inspect.signature(sc.build_graph_device).parameters["broad_phase"].default == "host"
    assert inspect.signature(sc.graph_from_sets_device).parameters["broad_phase"].default == "host"
    As, bs = _four_boxes()
    with pytest.raises(ValueError, match="broad_phase"):
        sc.build_graph_device(As, bs, scene=FakeDeviceScene("ok"), broad_phase="grid")

    class HostOnly:                      # the interface of PolytopeScene: what the default must keep calling
        def centers(self): return FakeDeviceScene("ok").centers()
        def bounds(self, cen): return FakeDeviceScene("ok").bounds()[:2] + (np.zeros((4, 2, 2), np.int32),)
        def overlaps(self, pa, pb, tol, cen):
            return np.array([1 if (a, b) in {(0, 1), (1, 2)} else 0 for a, b in zip(pa.tolist(), pb.tolist())], np.uint8), np.zeros(len(pa), np.int32)
    from gcs_admm_amd.graph import build_graph
    assert sc.build_graph_device(As, bs, scene=HostOnly())[1] == build_graph(As, bs)[1]


def test_device_scene_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    As, bs = _four_boxes()
    with pytest.raises(sc.GcsAdmmError, match="no HIP device"):
        sc.DeviceScene([(As[v], bs[v]) for v in As])
