"""The bits the workgroup vertex program leaves: 20 iterations of gcsadmm_run from the zero state on small graphs that take every path of
the program's task decode (degree-1 sides, a pipeline wavefront that owns two units, the BOX instantiations), written as one .npz.

    python tools/wg_bits_record.py --out tests/golden/wg_bits.npz       # the fixture: recorded ONCE, from the build a change starts from
    python tools/wg_bits_record.py --out /tmp/now.npz [--lib build.so]  # the same run on the build at hand (tests/test_gpu_wg_bits.py)

A change that touches no floating-point operation of the program (address arithmetic, register use, scheduling hints) must reproduce
the fixture byte for byte; the file carries the compiler's version, since bits are a property of compiler plus source."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERATIONS = 20
ARRAYS = ("xv", "zv", "yv", "copy", "mu", "zedge")
# (name, graph, state type, vertex program): the n = 2 graphs on the 512-thread ("workgroup") and the 256-thread build
CASES = [("benchmark1", "benchmark1", t, p) for t in ("f64", "f32") for p in ("workgroup", "workgroup256")] + \
        [("benchmark3", "benchmark3", "f64", p) for p in ("workgroup", "workgroup256")] + \
        [("lattice3x3_n3", ("lattice", 3), "f64", "workgroup"), ("lattice3x3_n6", ("lattice", 6), "f64", "workgroup")]


def case_id(c):
    return f"{c[0]}-{c[2]}-{c[3]}"


def compiler_version():
    from gcs_admm_amd import build
    return "\n".join(line for line in build.compiler_version().splitlines() if "version" in line)


def graph_of(spec):
    from gcs_admm_amd.cases import load_fixture
    from gcs_admm_amd.graph import lattice_boxes
    return lattice_boxes(3, 3, n=spec[1]) if isinstance(spec, tuple) else load_fixture(spec)[1]


def run_case(c):
    from gcs_admm_amd.solver import DeviceSolver
    s = DeviceSolver(graph_of(c[1]), state_dtype=c[2], device=0, program=c[3])
    try:
        q = s.query()
        assert q["num_workgroup_vertices"] > 0 and not q["num_waves"], q       # every generic vertex on the workgroup program
        s.reset()
        s.enqueue(ITERATIONS)
        s.torch.cuda.synchronize(s.device)
        out = {name: getattr(s, name).cpu().numpy().copy() for name in ARRAYS}
        out["trace"] = s.trace[:ITERATIONS].cpu().numpy().copy()
        assert np.isfinite(out["copy"]).all() and np.abs(out["copy"]).max() > 0
        return out
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--lib", help="a build of the library other than the in-tree one")
    args = ap.parse_args()
    if args.lib:
        from gcs_admm_amd import abi
        abi.select_library(args.lib)
    data = {"compiler": np.array(compiler_version())}
    for c in CASES:
        for name, arr in run_case(c).items():
            data[f"{case_id(c)}/{name}"] = arr
        print("recorded", case_id(c), flush=True)
    np.savez_compressed(args.out, **data)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
