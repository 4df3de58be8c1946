"""Host builds of an emulation source against copies of csrc/ with one seeded error each: the one builder of the "mutant" fixtures
(test_polytope_lp_mutants.py, test_path_restrict_mutants.py, test_solve_agreement_mutants.py, test_halo_plan.py)."""
import ctypes as C
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

from gcs_admm_amd.native_build import build_library
from hostemu_lib import BASE

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gcs_admm_amd", "csrc")


def build_mutants(base, header, mutants, source, flags=(), more=()):
    """{name: CDLL} of ``source`` built once per entry of ``mutants`` ({name: [(anchor in ``header``, replacement)]}), each against
    its own copy of csrc/ under ``base`` (the whole directory: headers include each other from their own) with the substitutions
    applied; that copy comes first on the include path, ``flags`` after it.  ``more``: further (source, extra flags) units linked into
    every variant.  The variants compile concurrently."""
    def one(name):
        csrc = os.path.join(base, name, "csrc")
        shutil.copytree(CSRC, csrc)
        text = open(os.path.join(csrc, header)).read()
        for old, new in mutants[name]:
            assert text.count(old) == 1, f"mutant {name}: anchor {old!r} does not occur exactly once in {header} -- update MUTANTS"
            text = text.replace(old, new)
        with open(os.path.join(csrc, header), "w") as f:
            f.write(text)
        try:
            return build_library(os.path.join(base, name, "libmutant.so"), [(source, []), *more], flags=[*BASE, "-I" + csrc, *flags],
                                 objdir=os.path.join(base, name))
        except RuntimeError as e:
            raise AssertionError(f"build of mutant {name} failed") from e
    with ThreadPoolExecutor(len(mutants)) as pool:
        return {name: C.CDLL(so) for name, so in zip(mutants, pool.map(one, mutants))}
