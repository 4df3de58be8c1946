"""The Python binding (gcs_admm_amd/abi.py) against include/gcsadmm.h: every prototype, the descriptor's fields and struct layouts, the
pointer width of every pointer argument, and the descriptor builder; the library loads with those prototypes on it (no compute calls:
this runs without a GPU), and the Python host refuses to run without the GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLES = ("gcsadmm_handle", "gcsadmm_scene")
SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "gcsadmm_status": ctypes.c_int32, "int64_t": ctypes.c_int64,
           "long": ctypes.c_long, "double": ctypes.c_double}


def header_text():
    """include/gcsadmm.h without comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcsadmm.h")).read(), flags=re.S)
    return "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))


def kind(decl, result=False):
    """the ctypes kind of a parameter declaration ("const double *q_dev") or of a result type ("const char *")"""
    decl = " ".join(decl.replace("*", " * ").split())
    if result and decl == "const char *":
        return ctypes.c_char_p
    if result and decl == "void":
        return None
    words = decl.split() if result else decl.split()[:-1]          # a parameter carries its name last
    if "*" in words or words[-1] in HANDLES:
        return ctypes.c_void_p
    assert len(words) == 1, decl
    return SCALARS[words[0]]


def declared_prototypes():
    """{name: (argument kinds, result kind)} of every function the header declares"""
    table = {}
    for result, name, params in re.findall(r"([\w\s\*]+?)\b(gcsadmm_\w+)\s*\(([^()]*)\)\s*;", header_text()):
        assert name not in table, name
        params = [] if params.strip() == "void" else params.split(",")
        table[name] = ([kind(q) for q in params], kind(result, result=True))
    return table


def test_prototypes_equal_header():
    """abi.PROTOTYPES is the header's table exactly: the same names, argument counts, kind at every position, result type"""
    from gcs_admm_amd import abi, solver
    header = declared_prototypes()
    assert len(header) >= 38
    assert sorted(abi.PROTOTYPES) == sorted(header)
    for name, (argtypes, restype) in header.items():
        assert (list(abi.PROTOTYPES[name][0]), abi.PROTOTYPES[name][1]) == (argtypes, restype), name
    assert solver.EXPORTS == abi.EXPORTS == list(abi.PROTOTYPES)


def test_library_declares_prototypes():
    """after load_library() every function of the table is on the library with the table's argtypes and restype"""
    from gcs_admm_amd import abi, build, solver
    build.build()
    lib = solver.load_library()
    assert lib is abi.load_library()
    for name, (argtypes, restype) in abi.PROTOTYPES.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and list(f.argtypes) == list(argtypes), name
        assert f.restype == restype, name


def test_pointer_arguments_keep_64_bits():
    """a raw address (``t.data_ptr()``, ``a.ctypes.data``) survives at every position the header declares as a pointer or a handle"""
    from gcs_admm_amd import abi
    address = (1 << 40) + 8
    echo = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p)(lambda p: p)      # a foreign call with that argtype, into Python
    assert echo(address) == address
    assert ctypes.c_int(address).value == 8                                     # what an undeclared argument would be cut to
    pointers = 0
    for name, (argtypes, _) in declared_prototypes().items():
        for i, k in enumerate(argtypes):
            if k is ctypes.c_void_p:
                assert abi.PROTOTYPES[name][0][i] is ctypes.c_void_p, (name, i)
                pointers += 1
    assert pointers >= 100


def test_graph_desc_fields_equal_header():
    from gcs_admm_amd import abi
    body = re.search(r"typedef struct gcsadmm_graph_desc \{(.*?)\} gcsadmm_graph_desc;", header_text(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        if decl.strip():            # "int32_t src, dst": the type is everything before the first name
            first, *more = decl.split(",")
            names += [first.split()[-1].strip("*")] + [m.strip(" *\n") for m in more]
    assert len(names) >= 28 and names == [f for f, _ in abi.GraphDesc._fields_]


def _memory(address, dtype, count):
    return np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(dtype) * count).from_address(address)).copy() if count else np.zeros(0, dtype)


def _descriptor_cases():
    from gcs_admm_amd.cases import load_fixture
    from gcs_admm_amd.graph import lattice_boxes
    from gcs_admm_amd.partition import build_partition, strip_owner
    _, g = load_fixture("test1")
    NI = int(g.inc_ptr[-1])
    yield "test1", g, None, (np.arange(NI) % 3 != 0).astype(np.uint8), (np.arange(g.num_edges) % 2).astype(np.uint8), 0.0, 0.0
    lat = lattice_boxes(4, 6)
    p = build_partition(lat, strip_owner(lat, 2), 0, 2)                  # ghost columns and the ownership masks of a real partition
    assert p.num_incidences > int(p.graph.inc_ptr[-1]) and p.inc_counted.min() == 0
    yield "lattice", p.graph, p.num_incidences, p.inc_counted, p.edge_counted, p.nx_global, p.nmu_global


@pytest.mark.parametrize("columns", ["incidence", "edge"])
def test_graph_desc_builder(columns):
    """abi.graph_desc against the arithmetic DeviceSolver.__init__ did before the builder existed, restated here in plain numpy: field
    values, the contents of every array the descriptor points to, and col_of -- with the edge-major renumbering of ``inc_counted``"""
    from gcs_admm_amd import abi
    knobs = dict(vertex_program=2, wave_slots=3, wave_align=1, wave_store_dl=2, wave_generic_rows=1, vertex_workspace=1)
    for name, g, num_inc, inc_counted, edge_counted, nx, nmu in _descriptor_cases():
        E, V = g.num_edges, g.num_vertices
        NI = int(g.inc_ptr[-1]) if num_inc is None else int(num_inc)
        tail, head = g.edge_inc_tail.astype(np.int32), g.edge_inc_head.astype(np.int32)
        col_of, ic = np.arange(NI, dtype=np.int64), np.asarray(inc_counted, dtype=np.uint8)
        if columns == "edge":
            assert NI == 2 * E
            col_of = np.empty(NI, dtype=np.int64)
            col_of[tail] = np.arange(E); col_of[head] = E + np.arange(E)
            tail, head = np.arange(E, dtype=np.int32), (E + np.arange(E)).astype(np.int32)
            ic_new = np.empty(NI, dtype=np.uint8)
            ic_new[col_of] = ic
            assert not np.array_equal(ic_new, ic), name                   # the renumbering moves the mask
            ic = ic_new
        scalars = dict(n=g.n, num_vertices=V, num_edges=E, num_incidences=NI, src=g.src, dst=g.dst, state_dtype=abi.F32, device=3,
                       nx_global=float(nx), nmu_global=float(nmu), edge_major_columns=int(columns == "edge"), **knobs)
        arrays = dict(inc_ptr=g.inc_ptr.astype(np.int32), inc_edge=g.inc_edge.astype(np.int32), inc_out=g.inc_out.astype(np.int32),
                      edge_inc_tail=tail, edge_inc_head=head, poly_ptr=g.poly_ptr.astype(np.int32),
                      poly_A=g.poly_A.astype(np.float64).ravel(), poly_b=g.poly_b.astype(np.float64).ravel(),
                      center=g.interior.astype(np.float64).ravel(), inc_counted=ic, edge_counted=np.asarray(edge_counted, dtype=np.uint8))
        assert set(scalars) | set(arrays) == {f for f, _ in abi.GraphDesc._fields_}

        d, keep, got_col_of = abi.graph_desc(g, state_dtype=abi.F32, device=3, num_incidences=num_inc, inc_counted=inc_counted,
                                              edge_counted=edge_counted, nx_global=nx, nmu_global=nmu, columns=columns, **knobs)
        for f, v in scalars.items():
            assert getattr(d, f) == v, (name, f)
        kept = {a.ctypes.data for a in keep if a is not None}
        for f, a in arrays.items():
            assert getattr(d, f) in kept, (name, f)
            got = _memory(getattr(d, f), a.dtype, a.size)
            assert got.dtype == a.dtype and np.array_equal(got, a), (name, f)
        assert got_col_of.dtype == np.int64 and np.array_equal(got_col_of, col_of), name
        # without masks the two pointers are null (= all counted)
        d0, _, _ = abi.graph_desc(g, state_dtype=abi.F64, device=0, num_incidences=num_inc, columns=columns)
        assert d0.inc_counted is None and d0.edge_counted is None and d0.vertex_program == 0 and d0.state_dtype == abi.F64


def _run(code):
    import subprocess
    import sys
    subprocess.check_call([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n" % ROOT + code])


def test_abi_imports_without_library(tmp_path):
    """gcs_admm_amd.abi imports without the library and without torch; a missing library is an error only when it is loaded, and
    after select_library both loaders (solver.load_library is abi's) name the selected path"""
    _run("from gcs_admm_amd import abi; assert 'torch' not in sys.modules and abi._lib is None\n"
         "abi.select_library(%r)\n"
         "from gcs_admm_amd import solver\n"
         "for load in (abi.load_library, solver.load_library):\n"
         "    try: load()\n"
         "    except RuntimeError as e: assert 'is missing' in str(e) and %r in str(e), e\n"
         "    else: raise SystemExit(1)" % (str(tmp_path / "none.so"), str(tmp_path / "none.so")))


def test_a_second_library_is_refused(tmp_path):
    """one library per process: after a load, select_library takes the loaded path again and refuses every other (a stand-in for the
    loaded library: the rule needs neither the build nor a GPU)"""
    _run("import ctypes\nfrom gcs_admm_amd import abi\n"
         "abi._lib = ctypes.CDLL(None); abi._lib._name = abi.LIB_PATH\n"
         "abi.select_library(abi.LIB_PATH)\n"
         "try: abi.select_library(%r)\n"
         "except RuntimeError as e: assert 'already loaded' in str(e) and abi.LIB_PATH in str(e), e\n"
         "else: raise SystemExit(1)\n"
         "assert abi.LIB_PATH.endswith('libgcsadmm.so')" % str(tmp_path / "other.so"))


def test_lib_path_is_read_in_abi_alone():
    """the package and the tools reach the library's path through abi.select_library / abi.load_library only"""
    seen = 0
    for top in ("gcs_admm_amd", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(".py") and os.path.join(top, f) != os.path.join("gcs_admm_amd", "abi.py"):
                    seen += 1
                    text = open(os.path.join(d, f)).read()
                    assert "LIB_PATH" not in text and "GCSADMM_PROBE_LIB" not in text and "GCSADMM_TIMING_LIB" not in text, os.path.join(d, f)
    assert seen > 40


def test_struct_layouts_match_header(tmp_path):
    """sizes and field offsets of the ctypes mirrors equal what a C compiler derives from include/gcsadmm.h"""
    import subprocess
    from gcs_admm_amd import solver
    pairs = [("gcsadmm_graph_desc", solver.GraphDesc), ("gcsadmm_params", solver.Params), ("gcsadmm_state", solver.State),
             ("gcsadmm_control_block", solver.ControlBlock), ("gcsadmm_halo_desc", solver.HaloDesc)]
    lines = []
    for cname, ct in pairs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gcsadmm.h"\nint main(void){' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, ct in pairs:
        assert int(got[cname]) == ctypes.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(ct, fname).offset, (cname, fname)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gcs_admm_amd.cases import load_fixture
    from gcs_admm_amd.solver import DeviceSolver
    _, g = load_fixture("test1")
    with pytest.raises(RuntimeError, match="no HIP device"):
        DeviceSolver(g)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "gcs_admm_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "libgcs_oracle" not in txt, f
