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
    for top in ("gcs_admm_amd", "tests", os.path.join("tools", "flopcount")):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(".py"):
                    yield os.path.join(d, f)
    yield os.path.join(ROOT, "tools", "fuzz_replay.py")


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
    assert seen > 50
    text = open(os.path.join(ROOT, "gcs_admm_amd", "build.py")).read()
    assert "subprocess" not in text and text.count("build_library(") == 2          # the product and build_timing
