"""What LOCATE_CHUNK (regions per workgroup of locate_kernel, csrc/point_locate_core.h) is measured against: the time of one
``DeviceScene.locate`` call for builds of the library with other chunk sizes, on the scenes of tools/query_bench.py.

  python tools/locate_chunk_sweep.py --build [--chunks 64 256 1024]     # compile the variants (no GPU needed)
  python tools/locate_chunk_sweep.py [--chunks 64 256 1024]             # time them: one fresh process per variant, two rounds, alternated

A variant is ``build.variant("locate_chunk", n=<c>)``: csrc/polytope_lp.hip compiled with -DGCS_LOCATE_CHUNK=<c> and linked with the
other objects of the in-tree build into gcs_admm_amd/libgcsadmm_chunk<c>.so.  Median of 51 calls after 5 warm-up calls, host clock (the call ends in a copy from the device).
One JSON line per (variant, round, scene, Q).
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def child(chunk, rnd):
    import numpy as np
    from gcs_admm_amd import abi, build
    abi.select_library(build.variant("locate_chunk", n=chunk))               # before the first load: every scene of this process runs the variant
    from bench_overlap import scene_polys
    from gcs_admm_amd.scene import DeviceScene
    for n, P in ((2, 1000), (2, 20000), (6, 1000)):
        rng = np.random.default_rng(n)
        polys = scene_polys(rng, n, P, 3 + n)
        with DeviceScene(polys) as scene:
            cen = scene.centers()[0]
            for Q in (2, 16, 128):
                jitter = np.zeros((Q, n)); jitter[:, :2] = rng.uniform(-0.2, 0.2, (Q, min(n, 2)))
                pts = cen[rng.integers(0, P, Q)] + jitter
                for _ in range(5):
                    hits = scene.locate(pts)
                ts = []
                for _ in range(51):
                    t0 = time.perf_counter(); scene.locate(pts); ts.append(time.perf_counter() - t0)
                print(json.dumps({"metric": "locate_call_s", "chunk": chunk, "round": rnd, "n": n, "regions": P, "points": Q,
                                  "median_s": float(np.median(ts)), "min_s": float(min(ts)), "hits": int(len(hits[1]))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, nargs="*", default=[64, 256, 1024])
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--child", type=int, nargs=2, metavar=("CHUNK", "ROUND"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if args.build:
        from gcs_admm_amd import build
        for c in args.chunks:
            print(build.variant("locate_chunk", n=c))
        return
    for rnd in range(2):
        for c in args.chunks:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(c), str(rnd)], timeout=120)


if __name__ == "__main__":
    main()
