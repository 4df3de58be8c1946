"""Measurement for the cover test of polylines (``DeviceScene.clip_segments``: segment_clip_kernel and segment_chain_kernel,
csrc/segment_clip_core.h): seconds per ``clip_segments`` call -- upload of the end points, count pass, scan on the host, fill pass, chain
kernel, read-back of the nine arrays -- on lattices of 1 000 and 20 000 overlapping cells in R^2, for 1, 8 and 64 polylines of 8
segments each (random walks with steps of up to two cells that stay inside the lattice's extent), against a vectorised numpy
implementation of the same rule (spans of all pairs as [segments, regions, rows] arrays, 32 segments at a time, then the greedy sweep per
segment) in the same run, the two alternated.  Medians of ``--reps`` calls after a warm-up call of each, with the spread; every device
time is a host clock around a call that ends in a copy from the device.  numpy has no fma, so its spans may differ from the device's in
the last bits: per line the largest difference and whether the statuses and chains agree.  One JSON line per (lattice, polylines).

  python tools/cover_bench.py [--regions 1000 20000] [--polylines 1 8 64] [--segments 8] [--reps 7]
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401  (HIP runtime first, see abi.load_library)
from gcs_admm_amd.scene import DeviceScene


def lattice(P):
    """(polys, nx, ny): nx x ny cells [i - 0.05, i + 1.05] x [j - 0.05, j + 1.05], nx ny >= P cut to P"""
    ny = max(int(np.sqrt(P / 2)), 1)
    nx = -(-P // ny)
    A = np.vstack([np.eye(2), -np.eye(2)])
    polys = [(A, np.array([i + 1.05, j + 1.05, -(i - 0.05), -(j - 0.05)])) for i in range(nx) for j in range(ny)][:P]
    return polys, nx, ny


def polylines(rng, count, segments, nx, ny):
    """``count`` random walks of ``segments`` steps, each step up to two cells per axis, clipped to the complete columns of the lattice"""
    hi = np.array([nx - 1.0, float(ny)])
    out = []
    for _ in range(count):
        pts = [rng.uniform(0.0, hi)]
        for _ in range(segments):
            pts.append(np.clip(pts[-1] + rng.uniform(-2.0, 2.0, 2), 0.0, hi))
        out.append(np.array(pts))
    return out


def numpy_clip(A, b, rows, start, end, tol, block=32):
    """the rule of csrc/segment_clip_core.h on regions of ``rows`` rows each (A [P rows, n], b [P rows]), without fma: per segment
    (regions hit, t_in, t_out, status, reach, chain as positions in its own list)"""
    absA, s = np.abs(A), np.abs(A).sum(axis=1)
    out = []
    for q0 in range(0, len(start), block):
        p = start[q0:q0 + block]
        d = end[q0:q0 + block] - p
        g, h = p @ A.T - b, d @ A.T
        mag = np.abs(b) + np.abs(p) @ absA.T + np.abs(d) @ absA.T
        c = (tol * s + 2.0 ** -40 * mag) - g
        with np.errstate(divide="ignore", invalid="ignore"):
            t = c / h
        shape = (len(p), -1, rows)
        hi = np.minimum(np.where(h > 0, t, np.inf).reshape(shape).min(axis=2), 1.0)
        lo = np.maximum(np.where(h < 0, t, -np.inf).reshape(shape).max(axis=2), 0.0)
        hit = (lo <= hi) & ~((h == 0) & (c < 0)).reshape(shape).any(axis=2)
        for k in range(len(p)):
            region = np.nonzero(hit[k])[0]
            t_in, t_out = lo[k, region], hi[k, region]
            cur, chain = 0.0, []
            while cur < 1.0:
                ok = np.nonzero((t_in <= cur) & (cur < t_out))[0]
                if len(ok) == 0:
                    break
                best = ok[np.argmax(t_out[ok])]      # (argmax: the first of equals)
                chain.append(int(best)); cur = float(t_out[best])
            out.append((region, t_in, t_out, 0 if cur >= 1.0 else 1, cur, chain))
    return out


def measure(P, counts, segments, reps, tol=1e-9):
    polys, nx, ny = lattice(P)
    A, b = np.vstack([a for a, _ in polys]), np.hstack([r for _, r in polys])
    rng = np.random.default_rng(P)
    clock = time.perf_counter
    with DeviceScene(polys) as scene:
        for count in counts:
            lines = polylines(rng, count, segments, nx, ny)
            start, end = np.concatenate([l[:-1] for l in lines]), np.concatenate([l[1:] for l in lines])
            scene.clip_segments(start, end, tol); numpy_clip(A, b, 4, start, end, tol)      # warm-up at this shape
            t_dev, t_np = [], []
            for _ in range(reps):                                                           # alternated
                t0 = clock(); res = scene.clip_segments(start, end, tol); t_dev.append(clock() - t0)
                t0 = clock(); ref = numpy_clip(A, b, 4, start, end, tol); t_np.append(clock() - t0)
            hit_ptr, region, _, t_in, t_out, status, reach, chain_ptr, chain = res
            same_list = all(np.array_equal(region[hit_ptr[q]:hit_ptr[q + 1]], ref[q][0]) for q in range(len(start)))
            same_chain = same_list and all(ref[q][3] == status[q] and [hit_ptr[q] + j for j in ref[q][5]] == chain[chain_ptr[q]:chain_ptr[q + 1]].tolist()
                                           for q in range(len(start)))
            diff = max([0.0] + [float(max(np.abs(t_in[hit_ptr[q]:hit_ptr[q + 1]] - ref[q][1]).max(), np.abs(t_out[hit_ptr[q]:hit_ptr[q + 1]] - ref[q][2]).max()))
                                for q in range(len(start)) if len(ref[q][0])]) if same_list else None
            print(json.dumps({"metric": "seconds_per_clip_segments_call", "n": 2, "regions": P, "polylines": count, "segments": int(len(start)), "repeats": reps,
                              "clip_call_s": float(np.median(t_dev)), "clip_call_s_spread": [float(min(t_dev)), float(max(t_dev))],
                              "numpy_s": float(np.median(t_np)), "numpy_s_spread": [float(min(t_np)), float(max(t_np))],
                              "numpy_over_device": float(np.median(t_np) / np.median(t_dev)),
                              "hits": int(len(region)), "hits_per_segment": len(region) / len(start), "chain_links": int(len(chain)),
                              "longest_chain": int(np.diff(chain_ptr).max()), "covered": int((status == 0).sum()), "gaps": int((status == 1).sum()),
                              "numpy_same_hits": bool(same_list), "numpy_same_status_and_chains": bool(same_chain), "numpy_span_diff_max": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, nargs="*", default=[1000, 20000])
    ap.add_argument("--polylines", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    for P in args.regions:
        measure(P, args.polylines, args.segments, args.reps)


if __name__ == "__main__":
    main()
