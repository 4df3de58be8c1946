"""The workgroup vertex program reproduces its recorded bits (tests/golden/wg_bits.npz, written once by tools/wg_bits_record.py from the
build BEFORE the Newton loop's scalars were taken out of the spill lanes): 20 iterations of gcsadmm_run from the zero state on
benchmark1 (degree-1 sides; f64 and f32), benchmark3 (degrees above 7: a pipeline wavefront owns two units) -- both on the 512- and the
256-thread build -- and a 3 x 3 box lattice at n = 3 and n = 6 (the BOX instantiations).  x_v, z_v, y_v, copy, mu, z_edge and the trace
rows, byte for byte: a change of address arithmetic, register use or scheduling hints must not move one bit.

The runs are made by the recorder itself in ONE child process under a time limit (a hang there ends the test, not the session); the
fixture carries the compiler's version, and the comparison is skipped under another compiler: bits are a property of compiler plus
source."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wg_bits_record as rec  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "wg_bits.npz")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    gold = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 200 * 1024
    if str(gold["compiler"]) != rec.compiler_version():
        pytest.skip(f"the fixture was recorded under another compiler: {str(gold['compiler'])!r}")
    out = str(tmp_path_factory.mktemp("wg_bits") / "now.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "wg_bits_record.py"), "--out", out],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return gold, np.load(out)


@pytest.mark.parametrize("case", rec.CASES, ids=rec.case_id)
def test_same_bits(runs, case):
    gold, now = runs
    for name in rec.ARRAYS + ("trace",):
        key = f"{rec.case_id(case)}/{name}"
        a, b = gold[key], now[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (key, int((a != b).sum()), "entries differ")


def test_fixture_has_exactly_the_cases():
    gold = np.load(GOLDEN)
    want = {f"{rec.case_id(c)}/{name}" for c in rec.CASES for name in rec.ARRAYS + ("trace",)} | {"compiler"}
    assert set(gold.files) == want
