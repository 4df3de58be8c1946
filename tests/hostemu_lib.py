"""Every host build of device code the tests load (sources: tests/hostemu), declared once: the default flags, and per library its
units and what it adds to the defaults.  The modules that use a library keep its prototypes; this module has the flags and the paths."""
import ctypes as C
import os

from gcs_admm_amd.build import CSRC, ROOT, T512
from gcs_admm_amd.native_build import build_library

HOSTEMU = os.path.join(ROOT, "tests", "hostemu")
BASE = ["-O1", "-std=c++17", "-fPIC"]          # mutant_build.py puts its copy of csrc/ behind these
FLAGS = BASE + ["-I" + CSRC]
INCLUDE = "-I" + os.path.join(ROOT, "include")
# the plan shims link the workgroup program's LDS sizing as vertex_wg.hip is built: at 256 and at 512 threads.  Shims with equal
# flags share the two objects.
SIZES = [("wg_sizes.cpp", []), ("wg_sizes.cpp", T512)]
_shim = lambda source, *extra: (SIZES + [(source, list(extra))], [INCLUDE])

# lib<name>.so: ([(source in tests/hostemu, its own flags)], flags after the defaults)
LIBRARIES = {
    "emu": ([("emu.cpp", [])], []),                                           # the wavefront vertex program
    "wgemu": ([("wg_emu.cpp", [])], []),                                      # the workgroup vertex program, tasks ascending
    "wgemu_rev": ([("wg_emu.cpp", ["-DGCS_WG_REVERSE"])], []),                # ... and descending
    "wgsplitemu": ([("wg_split_emu.cpp", [])], []),                           # its split form
    "wgsplitemu_rev": ([("wg_split_emu.cpp", ["-DGCS_WG_REVERSE"])], []),
    "termemu": ([("term_emu.cpp", [])], []),
    "walkemu": ([("walk_emu.cpp", [])], []),
    "lpemu": ([("lp_emu.cpp", [])], []),
    "sweepemu": ([("sweep_emu.cpp", [])], []),
    "locateemu": ([("locate_emu.cpp", [])], ["-ffp-contract=off"]),           # only the written fma calls fuse, as in the kernel
    "sceneeditemu": ([("scene_edit_emu.cpp", [])], []),
    "scenestageemu": ([("scene_stage_emu.cpp", [])], []),
    "querygraphemu": ([("query_graph_emu.cpp", [])], []),
    "informedemu": ([("informed_emu.cpp", [])], []),
    "restrictemu": ([("restrict_emu.cpp", [])], ["-O2", INCLUDE]),            # the last -O holds: this one is built at -O2
    "planemu": _shim("plan_emu.cpp"),
    "fusedplanemu": _shim("fused_plan_emu.cpp"),
    "haloplanemu": _shim("halo_plan_emu.cpp"),
    "batchplanemu": _shim("batch_plan_emu.cpp"),
    "planwsemu": _shim("plan_ws_emu.cpp", "-I" + HOSTEMU),
}


def sources(units):
    return [(os.path.join(HOSTEMU, source), flags) for source, flags in units]


def emu_path(name, out=None, more=()):
    """build lib<name>.so (or ``out``, with ``more`` flags last: the sanitizer builds) if it is stale; its path"""
    units, added = LIBRARIES[name]
    return build_library(out or os.path.join(HOSTEMU, f"lib{name}.so"), sources(units), flags=FLAGS + added + list(more))


_loaded = {}


def emu_library(name) -> C.CDLL:
    if name not in _loaded:
        _loaded[name] = C.CDLL(emu_path(name))
    return _loaded[name]
