"""Measurement for edits of a resident scene (gcsadmm_scene_add_regions / gcsadmm_scene_remove_regions in csrc/polytope_lp.hip;
``DeviceScene`` and ``SceneQueries`` ``.add_regions`` / ``.remove_regions``): seconds to add the last K = 1, 16, 256 regions of a lattice
scene of about 1 000 and 20 000 regions (``graph.lattice_boxes``), and to remove them again, against the only route without edits: a
new ``SceneQueries`` on the edited set.  Three clocks per line: the scene call alone (``DeviceScene``), the whole ``SceneQueries`` edit
(the scene call plus the host's edge arrays), and the rebuild.  An add is followed by the removal of what it added, so every repetition
starts from the same scene; the edge arrays after the add must equal the rebuild's, or the run stops.  Medians after a warm-up of every
side, host clocks around calls that end in a copy from the device; min and max are reported beside every median.

  python tools/scene_edit_bench.py [--lattices 25x40 100x200] [--adds 1 16 256]

What EDIT_CHUNK (targets per workgroup of cross_kernel, csrc/scene_edit_core.h) is measured against: the ``DeviceScene.add_regions``
call for builds of the library with other chunk sizes, on the same scenes.

  python tools/scene_edit_bench.py --build [--chunks 64 256 1024]      # compile the variants (no GPU needed)
  python tools/scene_edit_bench.py --sweep [--chunks 64 256 1024]      # time them: one fresh process per variant, two rounds, alternated

A variant is ``build.variant("edit_chunk", n=<c>)``: csrc/polytope_lp.hip compiled with -DGCS_EDIT_CHUNK=<c> and linked with the other
objects of the in-tree build into gcs_admm_amd/libgcsadmm_editchunk<c>.so.  One JSON line per measurement.
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lattice(spec):
    """the regions of ``lattice_boxes(nx, ny)`` as a list (its two terminals, small boxes, are regions like the others here)"""
    from gcs_admm_amd.graph import lattice_boxes
    nx, ny = (int(v) for v in spec.split("x"))
    g = lattice_boxes(nx, ny)
    return [(g.poly_A[g.poly_ptr[i]:g.poly_ptr[i + 1]], g.poly_b[g.poly_ptr[i]:g.poly_ptr[i + 1]]) for i in range(g.num_vertices)]


def stat(ts):
    import numpy as np
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def scene_calls(polys, K, warm, reps):
    """``DeviceScene.add_regions`` of the last K regions and ``remove_regions`` of the same, alone"""
    from gcs_admm_amd.scene import DeviceScene
    P = len(polys) - K
    gone = list(range(P, P + K))
    with DeviceScene(polys[:P]) as scene:
        scene.centers(); scene.bounds(); scene.candidate_pairs(); scene.overlaps()
        t_add, t_rem = [], []
        for r in range(warm + reps):
            ta, (_, _, _, counts) = timed(lambda: scene.add_regions(polys[P:]))
            tr, _ = timed(lambda: scene.remove_regions(gone))
            if r >= warm:
                t_add.append(ta); t_rem.append(tr)
    return t_add, t_rem, counts


def measure(spec, adds, warm=2, reps=11, rebuilds=5):
    import numpy as np
    import torch  # noqa: F401  (HIP runtime first, see abi.load_library)
    from gcs_admm_amd.queries import SceneQueries
    polys = lattice(spec)
    sets = lambda count: ({p: polys[p][0] for p in range(count)}, {p: polys[p][1] for p in range(count)})
    for K in adds:
        P = len(polys) - K
        t_add, t_rem, counts = scene_calls(polys, K, warm, reps)
        new = ({p: polys[p][0] for p in range(P, P + K)}, {p: polys[p][1] for p in range(P, P + K)})
        q_add, q_rem, t_new = [], [], []
        with SceneQueries(*sets(P), 2) as sq:
            for r in range(warm + reps):
                ta, _ = timed(lambda: sq.add_regions(*new))
                tail, head = sq.edge_tail.copy(), sq.edge_head.copy()
                tr, _ = timed(lambda: sq.remove_regions(list(new[0])))
                if r >= warm:
                    q_add.append(ta); q_rem.append(tr)
        for r in range(1 + rebuilds):
            t, ref = timed(lambda: SceneQueries(*sets(P + K), 2))
            with ref:
                if not (np.array_equal(ref.edge_tail, tail) and np.array_equal(ref.edge_head, head)):
                    raise SystemExit(f"{spec}, K = {K}: the edges after the add differ from the rebuild's")
            if r >= 1:
                t_new.append(t)
        line = {"metric": "scene_edit_s", "lattice": spec, "regions": P, "added": K, "new_pairs": counts["new_pairs"],
                "region_edges": int(len(tail)), "scene_add": stat(t_add), "scene_remove": stat(t_rem), "queries_add": stat(q_add),
                "queries_remove": stat(q_rem), "rebuild": stat(t_new), "edges_equal": True}
        line["rebuild_over_queries_add"] = line["rebuild"]["median_s"] / line["queries_add"]["median_s"]
        line["rebuild_over_queries_remove"] = line["rebuild"]["median_s"] / line["queries_remove"]["median_s"]
        print(json.dumps(line), flush=True)


def child(chunk, rnd, lattices, adds):
    import torch  # noqa: F401
    from gcs_admm_amd import abi, build
    abi.select_library(build.variant("edit_chunk", n=chunk))               # before the first load: every scene of this process runs the variant
    for spec in lattices:
        polys = lattice(spec)
        for K in adds:
            t_add, _, counts = scene_calls(polys, K, 3, 31)
            print(json.dumps({"metric": "scene_add_call_s", "chunk": chunk, "round": rnd, "lattice": spec, "regions": len(polys) - K, "added": K,
                              "new_pairs": counts["new_pairs"], **stat(t_add)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", nargs="*", default=["25x40", "100x200"])
    ap.add_argument("--adds", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--chunks", type=int, nargs="*", default=[64, 256, 1024])
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--child", type=int, nargs=2, metavar=("CHUNK", "ROUND"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child, args.lattices, args.adds)
    if args.build:
        from gcs_admm_amd import build
        for c in args.chunks:
            print(build.variant("edit_chunk", n=c))
        return
    if args.sweep:
        for rnd in range(2):
            for c in args.chunks:
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(c), str(rnd), "--lattices", *args.lattices,
                                       "--adds", *map(str, args.adds)], timeout=300)
        return
    for spec in args.lattices:
        measure(spec, args.adds)


if __name__ == "__main__":
    main()
