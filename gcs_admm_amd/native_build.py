"""The one place that runs a compiler: build_library() makes a shared library from (source, flags) units, for the product
(hipcc, gfx950) and for every host build of device code (g++).

Dependencies come from the compiler (-MMD), never from a list kept by hand.  Freshness is content, not time: beside every object and
every library lies a stamp with the dependency paths of its last successful build and a SHA-256 over its command lines and the bytes
of those dependencies.  Paths inside ``root`` enter stamp and hash relative to it, so a tree that was copied or moved stays fresh;
a changed flag, header or header of a header does not.  Objects are named by source and flags (``<root>/build/obj`` unless the unit
names its own), so two libraries that compile the same unit the same way share it."""
from __future__ import annotations

import hashlib
import os
import shlex
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAMP = ".stamp"
COMMANDS: list = []        # every command run, in order: an unchanged tree appends nothing


class BuildError(RuntimeError):
    pass


def _rel(text: str, root: str) -> str:
    return text.replace(root + os.sep, "")


def _digest(cmds, deps, root):
    """None when a dependency is gone"""
    h = hashlib.sha256()
    for cmd in cmds:
        h.update(_rel("\0".join(cmd), root).encode() + b"\n")
    for d in deps:
        try:
            data = open(os.path.join(root, d), "rb").read()
        except OSError:
            return None
        h.update(f"{d}\0{len(data)}\0".encode() + data)
    return h.hexdigest()


def _fresh(out, cmds, root, also=()):
    try:
        digest, *deps = open(out + STAMP).read().split("\n")
    except OSError:
        return None
    if all(os.path.exists(f) for f in (out, *also)) and digest == _digest(cmds, deps, root):
        return deps
    return None


def _stamp(out, cmds, deps, root):
    with open(out + STAMP, "w") as f:
        f.write("\n".join([_digest(cmds, deps, root)] + list(deps)))


def _unstamp(out):
    if os.path.exists(out + STAMP):
        os.remove(out + STAMP)


def _compile(cmd, obj, root, remarks, verbose):
    """one object, its stamp last; the dependency paths"""
    dfile = cmd[cmd.index("-MF") + 1]
    _unstamp(obj)
    COMMANDS.append(cmd)
    p = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if verbose:
        sys.stderr.write(p.stderr)
    try:
        if p.returncode != 0:
            raise BuildError(f"{os.path.basename(cmd[0])} failed on {cmd[cmd.index('-c') + 1]}:\n{p.stderr}")
        rule = open(dfile).read().replace("\\\n", " ")
    finally:
        if os.path.exists(dfile):
            os.remove(dfile)
    deps = sorted({_rel(os.path.abspath(d), root) for d in shlex.split(rule[rule.index(": ") + 2:])})
    if remarks:
        with open(obj + remarks, "w") as f:
            f.write(p.stderr)
    _stamp(obj, [cmd], deps, root)
    return deps


def version(compiler="g++") -> str:
    """what ``compiler --version`` prints (bits are a property of compiler plus source: tools/wg_bits_record.py)"""
    return subprocess.check_output([compiler, "--version"], text=True)


def command_lines(out, units, flags, compiler, link_flags, root, objdir):
    """([(compile command, object)], link command) of build_library"""
    jobs = []
    for src, extra, *obj in units:
        base = [compiler, *flags, *extra]
        src = os.path.abspath(str(src))
        key = hashlib.sha256(_rel("\0".join(base + [src]), root).encode()).hexdigest()[:16]
        obj = obj[0] if obj else os.path.join(objdir, f"{os.path.splitext(os.path.basename(src))[0]}-{key}.o")
        jobs.append((base + ["-MMD", "-MF", obj + ".d", "-c", src, "-o", obj], obj))
    return jobs, [compiler, *(link_flags if link_flags is not None else [*flags, "-shared"]), *(o for _, o in jobs), "-o", out]


def build_library(out, units, flags=(), compiler="g++", link_flags=None, root=ROOT, objdir=None, remarks=None, force=False, verbose=False):
    """Build the shared library ``out`` and return its path.  units: (source, extra flags) or (source, extra flags, object path);
    each is compiled with ``flags`` + its extra flags, all stale ones concurrently, then linked with ``link_flags`` (default: ``flags``
    and -shared).  remarks: a suffix; the compiler's stderr of each unit is kept at <object><suffix> (hipcc's resource remarks).
    A failed compile raises BuildError with the compiler's message and leaves no stamp."""
    out, root = os.path.abspath(str(out)), os.path.abspath(str(root))
    jobs, link = command_lines(out, units, flags, compiler, link_flags, root, str(objdir) if objdir else os.path.join(root, "build", "obj"))
    cmds = [c for c, _ in jobs] + [link]
    if not force and _fresh(out, cmds, root) is not None:
        return out
    _unstamp(out)
    deps = [None if force else _fresh(obj, [cmd], root, also=[obj + remarks] if remarks else []) for cmd, obj in jobs]
    stale = [i for i, d in enumerate(deps) if d is None]
    for i in stale:
        os.makedirs(os.path.dirname(jobs[i][1]), exist_ok=True)
    if stale:
        with ThreadPoolExecutor(len(stale)) as pool:
            futures = [pool.submit(_compile, *jobs[i], root, remarks, verbose) for i in stale]
        for i, f in zip(stale, futures):
            deps[i] = f.result()
    COMMANDS.append(link)
    p = subprocess.run(link, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise BuildError(f"{os.path.basename(compiler)} failed to link {out}:\n{p.stderr}")
    _stamp(out, cmds, sorted(set().union(*deps)), root)
    return out
