"""Build the in-tree HIP library (gfx950 only):  python -m gcs_admm_amd.build"""
from __future__ import annotations

import os
import shutil
import sys

from .native_build import build_library

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
MAIN = os.path.join(CSRC, "gcsadmm.hip")
WG = os.path.join(CSRC, "vertex_wg.hip")        # workgroup-cooperative vertex program (n = 2, 3, 6; own object)
WGD = os.path.join(CSRC, "vertex_wg_dims.hip")  # the same program for n = 1, 4, 5, 7, 8 (own object: the builds run in parallel)
LP = os.path.join(CSRC, "polytope_lp.hip")      # batched tiny LPs for graph construction (own object, own dependencies)
TERM = os.path.join(CSRC, "terminal_region.hip")  # x-update of terminals that are regions (own object)
WALK = os.path.join(CSRC, "path_walk.hip")      # the rounding step's candidate walks (own object, own entry points)
# (source, object name, extra flags)
# vertex_wg.hip is built twice: 256 threads per workgroup, and 512 for launches of at most one workgroup per CU (own namespace and entry points)
T512 = ["-DGCS_WG_THREADS=512", "-Dgcs_wg=gcs_wg_t512", "-DGCS_WG_SYM(name)=name##_t512"]
UNITS = [(MAIN, "gcsadmm.o", []), (WG, "vertex_wg.o", []), (WG, "vertex_wg_t512.o", T512), (WGD, "vertex_wg_dims.o", []), (WGD, "vertex_wg_dims_t512.o", T512),
         (LP, "polytope_lp.o", []), (TERM, "terminal_region.o", []), (WALK, "path_walk.o", [])]
OUT = os.path.join(HERE, "libgcsadmm.so")


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


# the compiler's per-kernel resource remarks (registers, scratch, LDS) are kept next to each object: kernel_resources()
FLAGS = ["-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
LINK = ["--offload-arch=gfx950", "-shared", "-fPIC"]
_units = lambda names: [(src, extra, os.path.join(HERE, name)) for src, name, extra in UNITS if name in names]


def build(force: bool = False, verbose: bool = False) -> str:
    """The objects are compiled concurrently, then linked (native_build: dependencies from the compiler, freshness by content)."""
    return build_library(OUT, _units([name for _, name, _ in UNITS]), flags=FLAGS, compiler=hipcc(), link_flags=LINK,
                         remarks=".resources.txt", force=force, verbose=verbose)


def kernel_resources() -> dict:
    """{kernel name: {"vgprs": .., "agprs": .., "scratch": bytes per lane, "lds": static bytes}} of the last build, from the
    compiler's resource remarks."""
    import re
    build()
    out = {}
    for _, name, _ in UNITS:
        cur = None
        for line in open(os.path.join(HERE, name) + ".resources.txt"):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            if cur is None:
                continue
            for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
                m = re.search(pat, line)
                if m:
                    cur[key] = int(m.group(1))
    return out


def build_timing() -> str:
    """Diagnostic library (tools/wg_phase_timing.py): the workgroup program with its region stamps compiled in -- the 512-thread object
    (the one small graphs such as benchmark4 run) and, under its own symbol names, nothing else: the 256-thread object stays the product's."""
    units = _units(("gcsadmm.o", "polytope_lp.o", "vertex_wg.o", "vertex_wg_dims.o", "vertex_wg_dims_t512.o")) + [
        (WG, T512 + ["-DGCS_WG_TIMING"], os.path.join(HERE, "vertex_wg_t512_timing.o")),
        (TERM, ["-DGCS_TERM_TIMING"], os.path.join(HERE, "terminal_region_timing.o"))]       # the region-terminal solve with its phase stamps (tools/term_phase_timing.py)
    return build_library(os.path.join(HERE, "libgcsadmm_timing.so"), units, flags=FLAGS, compiler=hipcc(), link_flags=LINK, remarks=".resources.txt")


if __name__ == "__main__":
    if "--timing" in sys.argv:
        print(build_timing())
        sys.exit(0)
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
