"""Diagnostic: share of wave cycles per barrier-separated phase of the vertex kernel, from the -DGCS_PHASE_TIMING build
(python -m gcs_admm_amd.build --variant phase).  Read its SHARES, not its length.
usage: python tools/phase_timing.py [s10k] [benchmark4]      (default: both)"""
import sys, os, ctypes as C, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gcs_admm_amd import abi, build, solver
abi.select_library(build.variant("phase"))
from gcs_admm_amd.graph import lattice_boxes
from gcs_admm_amd.cases import load_fixture
names = ["setup", "targets", "dT:reduce", "decide", "start point",
         "passA+blockfactor+3 chunk reductions", "border_factor+affine", "passB+reduce", "border_sigma", "corr_rhs+reduce",
         "border_corr_solve", "passD+reduce", "border_alpha", "update(passE)"]
for wl in sys.argv[1:] or ("s10k", "benchmark4"):
    g = lattice_boxes(100, 100, seed=0) if wl == "s10k" else load_fixture("benchmark4")[1]
    d = solver.DeviceSolver(g, "f32" if wl == "s10k" else "f64", device=0, program="wavefront", columns="edge" if wl == "s10k" else "incidence")
    d.reset(max_it=1000, eps_abs=0.0, eps_rel=0.0)
    d.enqueue(160 if wl == "s10k" else 80)
    torch.cuda.synchronize()
    out = (C.c_ulonglong * 64)()
    before = np.zeros(64)
    d.lib.gcsadmm_debug_phase_cycles(out); before = np.array(list(out), dtype=np.float64)
    d.enqueue(20); torch.cuda.synchronize()
    d.lib.gcsadmm_debug_phase_cycles(out); cyc = np.array(list(out), dtype=np.float64) - before
    tot = cyc.sum()
    print(wl, "total wave-cycles (s_memtime ticks) over 20 steps: %.3e" % tot)
    print("  inner failures of the stamped kernels (they use scratch, profiles/diagnostic_builds): %d" % d.read_control().inner_failures)
    for i, n in enumerate(names):
        print("  %-28s %6.2f %%" % (n, 100 * cyc[i] / tot))
    sub = (C.c_ulonglong * 16)()
    d.lib.gcsadmm_debug_sub_cycles(sub)
    sv = np.array(list(sub), dtype=np.float64)
    if sv.sum() > 0:
        lab = ["", "cone scaling, W^-2", "sides: chol5, inverse, Y", "M: x-x block", "M: zeta-x, zeta-zeta, Su", "change of variables", "chol9", "store factor", "both solves: rhs + side products", "both solves: chol_solve + t", "affine solve: dnu + stores", "corrector solve: dnu + stores"]
        print("  inside border_factor (lane 0 of each wavefront, cumulative since start):")
        for k in range(1, 12):
            print("    %-28s %6.2f %%" % (lab[k], 100 * sv[k] / sv[1:12].sum()))
