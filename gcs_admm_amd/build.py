"""Build the in-tree HIP library (gfx950 only):  python -m gcs_admm_amd.build"""
from __future__ import annotations

import os
import shutil
import sys

from . import native_build

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


def compiler_version() -> str:
    return native_build.version(compiler=hipcc())


# the compiler's per-kernel resource remarks (registers, scratch, LDS) are kept next to each object: kernel_resources()
FLAGS = ["-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
LINK = ["--offload-arch=gfx950", "-shared", "-fPIC"]


def _library(out, units, **kw) -> str:
    """The objects are compiled concurrently, then linked (native_build: dependencies from the compiler, freshness by content)."""
    return native_build.build_library(out, units, flags=FLAGS, compiler=hipcc(), link_flags=LINK, remarks=".resources.txt", **kw)


def build(force: bool = False, verbose: bool = False) -> str:
    return _library(*_units(), force=force, verbose=verbose)


# Diagnostic builds.  name -> parameters -> (suffix of the library and of the changed objects, {object of UNITS: flags added to its own}).
# A variant compiles the named units again, as <unit>_<suffix>.o, and links them after the product's objects of every other unit.
_WG_OBJECT = {256: "vertex_wg.o", 512: "vertex_wg_t512.o"}
VARIANTS = {
    # the workgroup program with its region stamps, in the 512-thread object (the one small graphs such as benchmark4 run), and the
    # region-terminal solve with its phase stamps: tools/wg_phase_timing.py, tools/term_phase_timing.py
    "timing": lambda: ("timing", {"vertex_wg_t512.o": ["-DGCS_WG_TIMING"], "terminal_region.o": ["-DGCS_TERM_TIMING"]}),
    # the wavefront program with its phase stamps: tools/phase_timing.py
    "phase": lambda: ("phase", {"gcsadmm.o": ["-DGCS_PHASE_TIMING"]}),
    # two clock reads per solve of the workgroup program, in one of its two objects: tools/wg_blocktime.py
    "blocktime": lambda threads=512: (f"blocktime{int(threads)}", {_WG_OBJECT[int(threads)]: ["-DGCS_WG_BLOCKTIME"]}),
    # part k of the wavefront program's border factorisation executed twice: tools/variant_time.py
    "dup": lambda k: (f"dup{int(k)}", {"gcsadmm.o": [f"-DGCS_DUP={int(k)}"]}),
    # other chunk sizes of locate_kernel and of the scene-edit kernels: tools/locate_chunk_sweep.py, tools/scene_edit_bench.py
    "locate_chunk": lambda n: (f"chunk{int(n)}", {"polytope_lp.o": [f"-DGCS_LOCATE_CHUNK={int(n)}"]}),
    "edit_chunk": lambda n: (f"editchunk{int(n)}", {"polytope_lp.o": [f"-DGCS_EDIT_CHUNK={int(n)}"]}),
}


def _units(variant: str | None = None, **params):
    """(library, [(source, flags, object)]) of the product (None) or of a variant"""
    units = [(src, extra, os.path.join(HERE, name)) for src, name, extra in UNITS]
    if variant is None:
        return OUT, units
    suffix, added = VARIANTS[variant](**params)
    assert set(added) <= {name for _, name, _ in UNITS}, added
    again = [(src, extra + added[name], os.path.join(HERE, f"{name[:-2]}_{suffix}.o")) for src, name, extra in UNITS if name in added]
    return os.path.join(HERE, f"libgcsadmm_{suffix}.so"), [u for u, (_, name, _) in zip(units, UNITS) if name not in added] + again


def variant(name: str, **params) -> str:
    """Build gcs_admm_amd/libgcsadmm_<suffix>.so of VARIANTS[name] and return its path (abi.select_library takes it)."""
    return _library(*_units(name, **params))


def kernel_resources(variant: str | None = None, **params) -> dict:
    """{kernel name: {"vgprs": .., "agprs": .., "scratch": bytes per lane, "lds": static bytes}} of the last build of the product
    (or of a variant), from the compiler's resource remarks."""
    import re
    _, units = _units(variant, **params)
    _library(_, units)
    out = {}
    for _, _, obj in units:
        cur = None
        for line in open(obj + ".resources.txt"):
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


if __name__ == "__main__":
    args = ["--variant", "timing"] if "--timing" in sys.argv else sys.argv[1:]
    if "--variant" in args:
        at = args.index("--variant")
        print(variant(args[at + 1], **dict(kv.split("=", 1) for kv in args[at + 2:])))
    else:
        print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
