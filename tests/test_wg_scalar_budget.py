"""Scalar budget of the workgroup vertex program ("scalar budget of the Newton loop"), read from the compiler's
resource remarks of the in-tree build -- no GPU needed.  The Newton loop of csrc/vertex_wg.h keeps its uniform sizes opaque per region
(wg_opaque), so that what is derived from them is recomputed where it is used instead of living in a scalar register, or in a lane of a
spill register, for the whole loop.  A change that lets the loop-invariant hoister make those values live again shows up here as a
jump of the "SGPRs Spill" figure long before it shows up in a timing."""
import os
import re

# the n = 2 kernel the headline runs (benchmark4: 512 threads) and its 256-thread twin, f64 and f32: what this change reached
# (the commit before it: 184 in all four)
N2_BOUND = {"vertex_wg_t512": 32, "vertex_wg": 34}
N2_BEFORE = 184

# "SGPRs Spill" of every other vertex_wg_* kernel at the commit before this change: (object, kernel, n, state type, BOX) -> figure
BEFORE = {
    ("vertex_wg", "vertex_wg_batch_kernel", 2, "d", 0): 182,
    ("vertex_wg", "vertex_wg_batch_kernel", 2, "f", 0): 182,
    ("vertex_wg", "vertex_wg_batch_kernel", 3, "d", 0): 212,
    ("vertex_wg", "vertex_wg_batch_kernel", 3, "d", 1): 195,
    ("vertex_wg", "vertex_wg_batch_kernel", 3, "f", 0): 213,
    ("vertex_wg", "vertex_wg_batch_kernel", 3, "f", 1): 195,
    ("vertex_wg", "vertex_wg_batch_kernel", 6, "d", 0): 223,
    ("vertex_wg", "vertex_wg_batch_kernel", 6, "d", 1): 212,
    ("vertex_wg", "vertex_wg_batch_kernel", 6, "f", 0): 222,
    ("vertex_wg", "vertex_wg_batch_kernel", 6, "f", 1): 210,
    ("vertex_wg", "vertex_wg_kernel", 2, "d", 0): 184,
    ("vertex_wg", "vertex_wg_kernel", 2, "f", 0): 184,
    ("vertex_wg", "vertex_wg_kernel", 3, "d", 0): 212,
    ("vertex_wg", "vertex_wg_kernel", 3, "d", 1): 201,
    ("vertex_wg", "vertex_wg_kernel", 3, "f", 0): 212,
    ("vertex_wg", "vertex_wg_kernel", 3, "f", 1): 201,
    ("vertex_wg", "vertex_wg_kernel", 6, "d", 0): 228,
    ("vertex_wg", "vertex_wg_kernel", 6, "d", 1): 208,
    ("vertex_wg", "vertex_wg_kernel", 6, "f", 0): 228,
    ("vertex_wg", "vertex_wg_kernel", 6, "f", 1): 208,
    ("vertex_wg", "vertex_wg_split_kernel", 2, "d", 0): 160,
    ("vertex_wg", "vertex_wg_split_kernel", 2, "f", 0): 160,
    ("vertex_wg", "vertex_wg_split_kernel", 3, "d", 0): 195,
    ("vertex_wg", "vertex_wg_split_kernel", 3, "d", 1): 200,
    ("vertex_wg", "vertex_wg_split_kernel", 3, "f", 0): 195,
    ("vertex_wg", "vertex_wg_split_kernel", 3, "f", 1): 200,
    ("vertex_wg", "vertex_wg_split_kernel", 6, "d", 0): 223,
    ("vertex_wg", "vertex_wg_split_kernel", 6, "d", 1): 212,
    ("vertex_wg", "vertex_wg_split_kernel", 6, "f", 0): 223,
    ("vertex_wg", "vertex_wg_split_kernel", 6, "f", 1): 212,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 1, "d", 0): 151,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 1, "f", 0): 151,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 4, "d", 0): 184,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 4, "f", 0): 184,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 5, "d", 0): 181,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 5, "f", 0): 181,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 7, "d", 0): 245,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 7, "f", 0): 245,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 8, "d", 0): 184,
    ("vertex_wg_dims", "vertex_wg_batch_kernel", 8, "f", 0): 184,
    ("vertex_wg_dims", "vertex_wg_kernel", 1, "d", 0): 155,
    ("vertex_wg_dims", "vertex_wg_kernel", 1, "f", 0): 155,
    ("vertex_wg_dims", "vertex_wg_kernel", 4, "d", 0): 187,
    ("vertex_wg_dims", "vertex_wg_kernel", 4, "f", 0): 187,
    ("vertex_wg_dims", "vertex_wg_kernel", 5, "d", 0): 196,
    ("vertex_wg_dims", "vertex_wg_kernel", 5, "f", 0): 196,
    ("vertex_wg_dims", "vertex_wg_kernel", 7, "d", 0): 251,
    ("vertex_wg_dims", "vertex_wg_kernel", 7, "f", 0): 251,
    ("vertex_wg_dims", "vertex_wg_kernel", 8, "d", 0): 213,
    ("vertex_wg_dims", "vertex_wg_kernel", 8, "f", 0): 217,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 1, "d", 0): 153,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 1, "f", 0): 153,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 4, "d", 0): 168,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 4, "f", 0): 168,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 5, "d", 0): 185,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 5, "f", 0): 185,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 7, "d", 0): 242,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 7, "f", 0): 242,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 8, "d", 0): 187,
    ("vertex_wg_dims", "vertex_wg_split_kernel", 8, "f", 0): 187,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 1, "d", 0): 155,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 1, "f", 0): 155,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 4, "d", 0): 187,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 4, "f", 0): 187,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 5, "d", 0): 196,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 5, "f", 0): 196,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 7, "d", 0): 249,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 7, "f", 0): 249,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 8, "d", 0): 199,
    ("vertex_wg_dims_t512", "vertex_wg_kernel", 8, "f", 0): 201,
    ("vertex_wg_t512", "vertex_wg_kernel", 2, "d", 0): 184,
    ("vertex_wg_t512", "vertex_wg_kernel", 2, "f", 0): 184,
    ("vertex_wg_t512", "vertex_wg_kernel", 3, "d", 0): 217,
    ("vertex_wg_t512", "vertex_wg_kernel", 3, "d", 1): 196,
    ("vertex_wg_t512", "vertex_wg_kernel", 3, "f", 0): 218,
    ("vertex_wg_t512", "vertex_wg_kernel", 3, "f", 1): 196,
    ("vertex_wg_t512", "vertex_wg_kernel", 6, "d", 0): 229,
    ("vertex_wg_t512", "vertex_wg_kernel", 6, "d", 1): 211,
    ("vertex_wg_t512", "vertex_wg_kernel", 6, "f", 0): 229,
    ("vertex_wg_t512", "vertex_wg_kernel", 6, "f", 1): 211,
}


def _spills():
    from gcs_admm_amd import build
    build.build()
    out = {}
    for _, name, _ in build.UNITS:
        if not name.startswith("vertex_wg"):
            continue
        obj, cur = name[:-2], None
        for line in open(os.path.join(build.HERE, name) + ".resources.txt"):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                k = re.search(r"(vertex_wg(?:_split|_batch)?_kernel)ILi(\d)E([df])Lb([01])E", m.group(1))
                cur = (obj, k.group(1), int(k.group(2)), k.group(3), int(k.group(4))) if k else None
                if cur:
                    out[cur] = {}
                continue
            if cur is None:
                continue
            for key, pat in (("spill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
                m = re.search(pat, line)
                if m:
                    out[cur][key] = int(m.group(1))
    return out


def test_every_kernel_of_the_table_is_built():
    assert set(_spills()) == set(BEFORE)


def test_n2_kernels_keep_their_scalars_out_of_spill_lanes():
    seen = 0
    for k, v in _spills().items():
        if k[1] == "vertex_wg_kernel" and k[2] == 2:
            seen += 1
            assert BEFORE[k] == N2_BEFORE
            assert v["spill"] <= N2_BOUND[k[0]] < N2_BEFORE, (k, v)
    assert seen == 4, seen


def test_no_kernel_spills_more_scalars_than_before():
    for k, v in _spills().items():
        assert v["spill"] <= BEFORE[k], (k, v, BEFORE[k])


def test_no_scratch():
    for k, v in _spills().items():
        assert v["scratch"] == 0, (k, v)
