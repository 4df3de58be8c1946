"""gcs_admm_amd/native_build.py on a toy project (toy.cpp including toy.h) in a temporary directory: what counts as fresh -- the
content of the dependencies the compiler reports and the command lines, never a file time or the place of the tree -- and that no
other file of the repository runs a compiler."""
import ctypes as C
import os
import re
import shutil

import pytest

from gcs_admm_amd import native_build as nb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O0", "-std=c++17", "-fPIC"]


def project(root, value=1):
    root.mkdir()
    (root / "toy.h").write_text(f"#define TOY_VALUE {value}\n")
    (root / "toy.cpp").write_text('#include "toy.h"\n#ifndef TOY_SCALE\n#define TOY_SCALE 1\n#endif\nextern "C" int toy() { return TOY_VALUE * TOY_SCALE; }\n')
    return root


def build(root, flags=FLAGS, name="libtoy.so", extra=()):
    """(the library's path, the commands this call ran)"""
    before = len(nb.COMMANDS)
    out = nb.build_library(root / name, [(root / "toy.cpp", list(extra))], flags=flags, root=root)
    return out, nb.COMMANDS[before:]


def value(path):
    """(a copy is loaded: dlopen would hand back the library already loaded from the same path)"""
    copy = f"{path}.{len(os.listdir(os.path.dirname(path)))}.so"
    shutil.copy(path, copy)
    return C.CDLL(copy).toy()


def compiles(cmds):
    return [c for c in cmds if "-c" in c]


def test_a_second_call_runs_nothing(tmp_path):
    root = project(tmp_path / "p")
    out, cmds = build(root)
    assert len(cmds) == 2 and value(out) == 1                  # one compile, one link
    assert all("-MMD" in c for c in compiles(cmds))
    assert build(root) == (out, [])


@pytest.mark.parametrize("sources", ["older", "newer"])
def test_file_times_do_not_matter(tmp_path, sources):
    root = project(tmp_path / "p")
    out, _ = build(root)
    t_out = 1_500_000_000
    t_src = t_out + (-1000 if sources == "older" else 1000)
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            os.utime(p, (t_src, t_src) if f in ("toy.h", "toy.cpp") else (t_out, t_out))
    assert build(root)[1] == []


def test_a_copied_tree_stays_fresh(tmp_path):
    root = project(tmp_path / "p")
    build(root)
    copy = tmp_path / "elsewhere" / "q"
    shutil.copytree(root, copy)
    out, cmds = build(copy)
    assert cmds == [] and out == str(copy / "libtoy.so")


def test_a_changed_header_rebuilds(tmp_path):
    root = project(tmp_path / "p")
    build(root)
    (root / "toy.h").write_text("#define TOY_VALUE 2\n")       # one byte, same length
    out, cmds = build(root)
    assert len(compiles(cmds)) == 1 and value(out) == 2
    assert build(root)[1] == []


def test_a_changed_flag_rebuilds(tmp_path):
    root = project(tmp_path / "p")
    build(root)
    out, cmds = build(root, flags=FLAGS + ["-DTOY_SCALE=3"])
    assert len(compiles(cmds)) == 1 and value(out) == 3
    out, cmds = build(root)                                    # the first flags again: their object is still there, the library is not theirs
    assert compiles(cmds) == [] and len(cmds) == 1 and value(out) == 1


def test_a_header_of_a_header_is_a_dependency(tmp_path):
    """the case a list kept by hand misses"""
    root = project(tmp_path / "p")
    build(root)
    (root / "inner.h").write_text("#define TOY_VALUE 4\n")
    (root / "toy.h").write_text('#include "inner.h"\n')
    out, cmds = build(root)
    assert len(compiles(cmds)) == 1 and value(out) == 4
    stamp = open(out + nb.STAMP).read().split("\n")[1:]
    assert stamp == ["inner.h", "toy.cpp", "toy.h"]            # relative to the root, from the compiler
    (root / "inner.h").write_text("#define TOY_VALUE 5\n")
    out, cmds = build(root)
    assert len(compiles(cmds)) == 1 and value(out) == 5


def test_a_failed_compile_raises_with_the_message_and_leaves_no_stamp(tmp_path):
    root = project(tmp_path / "p")
    build(root)
    (root / "toy.h").write_text("#define TOY_VALUE 6 +;\n")
    with pytest.raises(nb.BuildError, match=r"(?s)g\+\+ failed on .*toy\.cpp.*error: expected primary-expression before"):
        build(root)
    stamps = [f for d, _, files in os.walk(root) for f in files if f.endswith(nb.STAMP)]
    assert stamps == []
    before = len(nb.COMMANDS)
    with pytest.raises(nb.BuildError):                         # and the next call compiles again
        build(root)
    assert len(nb.COMMANDS) == before + 1
    (root / "toy.h").write_text("#define TOY_VALUE 6\n")
    out, cmds = build(root)
    assert len(cmds) == 2 and value(out) == 6


def test_equal_units_are_compiled_once(tmp_path):
    root = project(tmp_path / "p")
    (root / "other.cpp").write_text('extern "C" int other() { return 0; }\n')
    lib = lambda name, extra: nb.build_library(root / name, [(root / "toy.cpp", extra), (root / "other.cpp", [])], flags=FLAGS, root=root)
    before = len(nb.COMMANDS)
    lib("liba.so", [])
    lib("libb.so", [])
    toy = [c for c in compiles(nb.COMMANDS[before:]) if str(root / "toy.cpp") in c]
    assert len(toy) == 1
    lib("libc.so", ["-DTOY_EXTRA"])
    toy = [c for c in compiles(nb.COMMANDS[before:]) if str(root / "toy.cpp") in c]
    assert len(toy) == 2 and len(compiles(nb.COMMANDS[before:])) == 3          # other.cpp once for all three


# ---- structure: one helper ----
def _python_files():
    for top in ("gcs_admm_amd", "tests", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(".py"):
                    yield os.path.join(d, f)


def test_no_other_file_runs_a_compiler_or_compares_file_times():
    """outside native_build.py: no "g++" argument, hipcc() only handed on as the ``compiler`` of build_library, no getmtime"""
    me, helper = os.path.abspath(__file__), os.path.join(ROOT, "gcs_admm_amd", "native_build.py")
    seen = 0
    for path in _python_files():
        if path in (me, helper):
            continue
        seen += 1
        text = open(path).read()
        rel = os.path.relpath(path, ROOT)
        assert '"g++"' not in text and "'g++'" not in text, f"{rel} runs g++ itself"
        assert "getmtime" not in text, f"{rel} compares file times"
        for m in re.finditer(r"[^\n]*\bhipcc\(\)[^\n]*", text):
            line = m.group(0)
            assert re.search(r"compiler=(build\.)?hipcc\(\)|def hipcc\(\)", line), f"{rel}: {line.strip()}"
    assert seen > 90
    text = open(os.path.join(ROOT, "gcs_admm_amd", "build.py")).read()
    assert "subprocess" not in text and text.count("build_library(") == 1          # the product and every variant


def test_tools_do_not_name_the_compiler():
    """the scripts under tools/ build through gcs_admm_amd.build; the three that name hipcc describe a command for a person to run
    (micro/ holds stand-alone programs with their own build line, outside the package)"""
    named = set()
    for d, _, files in os.walk(os.path.join(ROOT, "tools")):
        for f in files:
            rel = os.path.relpath(os.path.join(d, f), os.path.join(ROOT, "tools"))
            if f.endswith((".py", ".sh", ".md")) and "hipcc" in open(os.path.join(d, f)).read():
                named.add(rel)
    assert named <= {"sanitize_cpu.sh", "wg_loop_stats.py", os.path.join("micro", "README.md")}
    code = open(os.path.join(ROOT, "tools", "wg_loop_stats.py")).read().split('"""')[2]
    assert "hipcc" not in code                                 # its docstring only


# ---- the variant table of build.py ----
VARIANTS = [("timing", {}), ("phase", {}), ("blocktime", {}), ("blocktime", {"threads": 256}), ("dup", {"k": 1}), ("locate_chunk", {"n": 64}),
            ("edit_chunk", {"n": 64})]
# variant -> {object of UNITS that is compiled again: (its new name, the flags added)}
EXPECTED = {
    "timing {}": ("libgcsadmm_timing.so", {"vertex_wg_t512.o": ("vertex_wg_t512_timing.o", ["-DGCS_WG_TIMING"]),
                                           "terminal_region.o": ("terminal_region_timing.o", ["-DGCS_TERM_TIMING"])}),
    "phase {}": ("libgcsadmm_phase.so", {"gcsadmm.o": ("gcsadmm_phase.o", ["-DGCS_PHASE_TIMING"])}),
    "blocktime {}": ("libgcsadmm_blocktime512.so", {"vertex_wg_t512.o": ("vertex_wg_t512_blocktime512.o", ["-DGCS_WG_BLOCKTIME"])}),
    "blocktime {'threads': 256}": ("libgcsadmm_blocktime256.so", {"vertex_wg.o": ("vertex_wg_blocktime256.o", ["-DGCS_WG_BLOCKTIME"])}),
    "dup {'k': 1}": ("libgcsadmm_dup1.so", {"gcsadmm.o": ("gcsadmm_dup1.o", ["-DGCS_DUP=1"])}),
    "locate_chunk {'n': 64}": ("libgcsadmm_chunk64.so", {"polytope_lp.o": ("polytope_lp_chunk64.o", ["-DGCS_LOCATE_CHUNK=64"])}),
    "edit_chunk {'n': 64}": ("libgcsadmm_editchunk64.so", {"polytope_lp.o": ("polytope_lp_editchunk64.o", ["-DGCS_EDIT_CHUNK=64"])}),
}


def _requested(monkeypatch, call):
    """what ``call`` hands to build_library, without building: (library, units, the other arguments)"""
    from gcs_admm_amd import build
    got = []
    monkeypatch.setattr(build, "hipcc", lambda: "hipcc")
    monkeypatch.setattr(nb, "build_library", lambda out, units, **kw: got.append((out, units, kw)) or out)
    call(build)
    return got[-1]


@pytest.mark.parametrize("name,params", VARIANTS, ids=["-".join([n] + [f"{k}{v}" for k, v in p.items()]) for n, p in VARIANTS])
def test_a_variant_differs_from_the_product_in_its_named_units_only(monkeypatch, name, params):
    from gcs_admm_amd import build
    _, product, how = _requested(monkeypatch, lambda b: b.build())
    out, units, how_v = _requested(monkeypatch, lambda b: b.variant(name, **params))
    library, changed = EXPECTED[f"{name} {params}"]
    assert out == os.path.join(build.HERE, library)
    assert {k: how_v[k] for k in ("flags", "compiler", "link_flags", "remarks")} == {k: how[k] for k in ("flags", "compiler", "link_flags", "remarks")}
    assert len(units) == len(product) == len(build.UNITS)
    want = [u for u, (_, obj, _) in zip(product, build.UNITS) if obj not in changed]
    want += [(src, extra + changed[obj][1], os.path.join(build.HERE, changed[obj][0])) for src, obj, extra in build.UNITS if obj in changed]
    assert units == want
    assert set(changed) <= {obj for _, obj, _ in build.UNITS}


def test_variant_parameters_are_checked():
    from gcs_admm_amd import build
    with pytest.raises(KeyError):
        build.variant("no_such_variant")
    with pytest.raises(TypeError):
        build._units("dup")                                    # k has no default
    with pytest.raises(KeyError):
        build._units("blocktime", threads=128)


# the command lines of the timing build as build_timing() gave them before the table (paths relative to the repository), with one
# change: the link line now names path_walk.o.  build_timing() left it out, so the library lacked the gcsadmm_walks_* entry points
# and abi.load_library, which declares every prototype, could not load it.
_F = "hipcc -Rpass-analysis=kernel-resource-usage --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -Igcs_admm_amd/csrc"
_T512 = "-DGCS_WG_THREADS=512 -Dgcs_wg=gcs_wg_t512 -DGCS_WG_SYM(name)=name##_t512"
_cc = lambda flags, src, obj: " ".join(filter(None, [_F, flags, f"-MMD -MF gcs_admm_amd/{obj}.d -c gcs_admm_amd/csrc/{src} -o gcs_admm_amd/{obj}"]))
TIMING_COMMANDS = [
    _cc("", "gcsadmm.hip", "gcsadmm.o"),
    _cc("", "vertex_wg.hip", "vertex_wg.o"),
    _cc("", "vertex_wg_dims.hip", "vertex_wg_dims.o"),
    _cc(_T512, "vertex_wg_dims.hip", "vertex_wg_dims_t512.o"),
    _cc("", "polytope_lp.hip", "polytope_lp.o"),
    _cc("", "path_walk.hip", "path_walk.o"),
    _cc(_T512 + " -DGCS_WG_TIMING", "vertex_wg.hip", "vertex_wg_t512_timing.o"),
    _cc("-DGCS_TERM_TIMING", "terminal_region.hip", "terminal_region_timing.o"),
    "hipcc --offload-arch=gfx950 -shared -fPIC gcs_admm_amd/gcsadmm.o gcs_admm_amd/vertex_wg.o gcs_admm_amd/vertex_wg_dims.o "
    "gcs_admm_amd/vertex_wg_dims_t512.o gcs_admm_amd/polytope_lp.o gcs_admm_amd/path_walk.o gcs_admm_amd/vertex_wg_t512_timing.o "
    "gcs_admm_amd/terminal_region_timing.o -o gcs_admm_amd/libgcsadmm_timing.so",
]


def test_timing_variant_runs_the_commands_it_always_did(monkeypatch):
    out, units, how = _requested(monkeypatch, lambda b: b.variant("timing"))
    jobs, link = nb.command_lines(out, units, how["flags"], how["compiler"], how["link_flags"], ROOT, None)
    assert [" ".join(c).replace(ROOT + os.sep, "") for c in [c for c, _ in jobs] + [link]] == TIMING_COMMANDS
    assert how["remarks"] == ".resources.txt"


# ---- every diagnostic macro of csrc/ has a recipe ----
# GCS_* names a preprocessor conditional of csrc/ may test without a build that sets them, each with its reason
ALLOWED = {
    "GCS_TAIL_WORDS": "tunable with a default in edge_step.h; no tool sweeps it",
    "GCS_WG_CONE_PAIR_MAXN": "tunable with a default in vertex_wg.h; no tool sweeps it",
    "GCS_STAMP": "internal: vertex_program.inc defines it itself, as a fence or as nothing",
    "GCS_NOFENCE": "mask of GCS_STAMP fences to drop; no tool uses it, so the table has no variant for it (tools/README.md)",
    "GCS_BOX": "instantiation parameter: vertex_program.h defines it around each inclusion of vertex_program.inc",
    "GCS_MFIX": "instantiation parameter, as GCS_BOX",
}


def test_every_macro_a_conditional_tests_has_a_recipe():
    import hostemu_lib
    from gcs_admm_amd import build
    tested = set()
    for f in os.listdir(build.CSRC):
        for line in open(os.path.join(build.CSRC, f)):
            m = re.match(r"\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)", line)
            if m:
                tested |= set(re.findall(r"\bGCS_\w+", m.group(1)))
    assert len(tested) >= 16
    macros = lambda flags: {m for f in flags for m in re.findall(r"^-D(GCS_\w+)", f)}
    product = set().union(*(macros(extra) for _, _, extra in build.UNITS))
    variants = set().union(*(macros(added) for name, params in VARIANTS for added in build.VARIANTS[name](**params)[1].values()))
    emulation = set().union(*(macros(added) | set().union(*(macros(own) for _, own in units)) for units, added in hostemu_lib.LIBRARIES.values()))
    assert {name for name, _ in VARIANTS} == set(build.VARIANTS)
    assert not set(ALLOWED) & (product | variants | emulation)
    assert tested - product - variants - emulation == set(ALLOWED)


# ---- the host-emulation table of tests/hostemu_lib.py ----
def test_every_emulation_library_is_used_and_declared_once():
    import hostemu_lib
    tests = {f: open(os.path.join(ROOT, "tests", f)).read() for f in os.listdir(os.path.join(ROOT, "tests")) if f.endswith(".py")}
    for name in hostemu_lib.LIBRARIES:
        users = [f for f, text in tests.items() if re.search(r"emu_(library|path)\(\"%s\"" % name, text)]
        assert users, f"no test asks for lib{name}.so"
    spelled = [f for f, text in tests.items() if '["-O1", "-std=c++17"' in text]
    assert sorted(spelled) == ["hostemu_lib.py", os.path.basename(__file__)]
